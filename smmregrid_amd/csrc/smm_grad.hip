// Source gradients on a regular lon/lat grid and the K-column apply (gfx950): what `method="bic"` and `method="con2"`
// weights need beyond their column 0.  Two kernels:
//   smm_gradients_kernel   a stencil: lanes along i, a workgroup walks a band of rows with the three source rows it
//                          needs in an LDS ring, f read once (plus two halo rows per band), every plane written once
//   smm_apply_cols_kernel  smm_apply_sell_kernel reading one column index and K weights per slot and gathering from f
//                          and the K - 1 planes at that column
// The rule is the text of include/smmregrid_amd.h ("weight columns and source gradients"); every multiply, subtract and
// add below is a rounded operation of its own (contraction is off), in the order that text and GradientRule state.
#include "smm_grad.hpp"

#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>

#include "smm_device.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kGradTileX = 256;      // columns per workgroup = threads
constexpr int kGradBandRows = 32;    // rows a workgroup walks: (32 + 2) / 32 of f is read

// f[j, gc] of one batch row as the stencil sees it, widened: NaN -- absent -- outside the grid; a periodic grid wraps
// the one column either side (gc == -1, gc == nx).  Every index formed lies in [0, nx * ny).
template <typename XT>
__device__ __forceinline__ double grad_cell(const XT* __restrict__ row, int nx, int ny, int periodic, int j, int gc) {
  int c = gc;
  bool in = j >= 0 && j < ny;
  if (c < 0 || c >= nx) {
    in = in && periodic && (c == -1 || c == nx);
    c = c < 0 ? nx - 1 : 0;
  }
  const int jc = min(max(j, 0), ny - 1);   // the load is unconditional: its index is clamped into the grid
  const double v = (double)row[(int64_t)jc * nx + c];
  return in ? v : __builtin_nan("");
}

// The difference rule along one axis at a cell: fc / fp / fm are f at the cell, its + and its - neighbour (presence), vc /
// vp / vm the values differenced (f itself, or the g_j plane for the cross term), s the axis' table of three scales
// (both sides, + only, - only) `stride` apart, m the row factor (ci[j]; 1.0 along j).
__device__ __forceinline__ double grad_diff(double fc, double fp, double fm, double vc, double vp, double vm,
                                            const double* __restrict__ s, int stride, int idx, double m) {
  const bool pp = __builtin_isfinite(fp), pm = __builtin_isfinite(fm);
  const bool ok = __builtin_isfinite(fc) && (pp || pm);
  const double hi = pp ? vp : vc, lo = pm ? vm : vc;
  const int code = (pp && pm) ? 0 : (pp ? 1 : 2);
  const double d = hi - lo;
  const double ds = d * s[code * stride + idx];
  const double dm = ds * m;
  return ok ? dm : 0.0;
}

template <typename XT>
__global__ __launch_bounds__(kGradTileX) void smm_gradients_kernel(GradArgs a) {
  // rows j - 1, j, j + 1 and the row being prefetched: four slots, so one barrier per row is enough (the slot written in
  // step j is none of the three read in step j - 1)
  __shared__ double ring[4][kGradTileX + 2];
  const int tid = threadIdx.x;
  uint32_t bid = blockIdx.x;
  const int xt = (int)(bid % (uint32_t)a.n_xtiles);
  bid /= (uint32_t)a.n_xtiles;
  const int band = (int)(bid % (uint32_t)a.n_bands);
  const int64_t b = bid / (uint32_t)a.n_bands;
  const XT* __restrict__ row = (const XT*)a.x + b * a.ldx;
  double* __restrict__ g = a.g + b * a.ld_row;
  const int nx = a.nx, ny = a.ny, periodic = a.periodic;
  const int i0 = xt * kGradTileX, i = i0 + tid;
  const int j0 = band * kGradBandRows, j1 = min(ny, j0 + kGradBandRows);
  // slot x of a ring row holds column i0 + x - 1: thread t fills slot t + 1, threads 0 and 1 the two halo slots too
  const bool halo = tid < 2;
  const int hslot = tid == 0 ? 0 : kGradTileX + 1;
  const int hcol = tid == 0 ? i0 - 1 : i0 + kGradTileX;
  auto slot = [](int j) { return (j + 1) & 3; };   // j >= -1
  for (int j = j0 - 1; j <= j0; ++j) {
    ring[slot(j)][tid + 1] = grad_cell(row, nx, ny, periodic, j, i);
    if (halo) ring[slot(j)][hslot] = grad_cell(row, nx, ny, periodic, j, hcol);
  }
  double nxt = grad_cell(row, nx, ny, periodic, j0 + 1, i);
  double nxt_h = halo ? grad_cell(row, nx, ny, periodic, j0 + 1, hcol) : 0.0;
  const int x = tid + 1;
  for (int j = j0; j < j1; ++j) {
    ring[slot(j + 1)][x] = nxt;
    if (halo) ring[slot(j + 1)][hslot] = nxt_h;
    if (j + 1 < j1) {   // the next step's row, in flight across the barrier and this step's arithmetic
      nxt = grad_cell(row, nx, ny, periodic, j + 2, i);
      if (halo) nxt_h = grad_cell(row, nx, ny, periodic, j + 2, hcol);
    }
    __syncthreads();
    if (i < nx) {
      const double* M = ring[slot(j - 1)];
      const double* C = ring[slot(j)];
      const double* P = ring[slot(j + 1)];
      const double fc = C[x], fe = C[x + 1], fw = C[x - 1];
      const double cij = a.ci[j];
      const double gi = grad_diff(fc, fe, fw, fc, fe, fw, a.si, nx, i, cij);
      const double gj = grad_diff(fc, P[x], M[x], fc, P[x], M[x], a.sj, ny, j, 1.0);
      const double gj_e = grad_diff(fe, P[x + 1], M[x + 1], fe, P[x + 1], M[x + 1], a.sj, ny, j, 1.0);
      const double gj_w = grad_diff(fw, P[x - 1], M[x - 1], fw, P[x - 1], M[x - 1], a.sj, ny, j, 1.0);
      const double gij = grad_diff(fc, fe, fw, gj, gj_e, gj_w, a.si, nx, i, cij);
      const int64_t at = (int64_t)j * nx + i;
      for (int p = 0; p < a.n_planes; ++p) {
        const int kind = a.kind[p];
        g[p * a.ld_plane + at] = kind == SMM_GRAD_I ? gi : (kind == SMM_GRAD_J ? gj : gij);
      }
    }
  }
}

// One destination row per lane, BT batch rows register-blocked, exactly as smm_apply_sell_kernel walks an operator; per
// slot one column index, K weights, and per batch row K gathers -- f (filled like any field) and the K - 1 planes.
template <typename XT, int K, int BT>
__global__ __launch_bounds__(kThreads) void smm_apply_cols_kernel(ColsArgs a, bool fill) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bid = blockIdx.x;
  const int64_t db = bid % a.n_dblocks;
  const int64_t jt = bid / a.n_dblocks;
  const int64_t slice = db * kWavesPerBlock + wave;
  const int64_t d = slice * 64 + lane;
  if (slice * 64 >= a.n_dst) return;

  const int64_t j0 = jt * BT;
  const XT* __restrict__ xr[BT];
  const double* __restrict__ gr[BT];
  double* __restrict__ yr[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    int64_t j = j0 + t;
    if (j > a.n_j - 1) j = a.n_j - 1;
    xr[t] = (const XT*)a.x + j * a.ldx;
    gr[t] = a.g + j * a.g_ld_row;
    yr[t] = a.y + j * a.ldy;
  }
  const int64_t off = a.slice_off[slice];
  const int nslots = (int)((a.slice_off[slice + 1] - off) >> 6);
  const int len = a.rowlen[d];
  const int32_t* __restrict__ cp = a.col + off + lane;
  const double* __restrict__ vp = a.val + off + lane;
  const double* __restrict__ xp = a.xval + off + lane;

  double acc[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) acc[t] = 0.0;
  // padded slots: a valid column, every weight +0.0 -- bitwise no-ops on a sum that is never -0.0 (smm_apply_sell_kernel)
#pragma unroll 2
  for (int k = 0; k < nslots; ++k) {
    const int32_t c = cp[(int64_t)k * 64];
    double w[K];
    w[0] = vp[(int64_t)k * 64];
#pragma unroll
    for (int q = 1; q < K; ++q) w[q] = xp[(int64_t)(q - 1) * a.n_slots + (int64_t)k * 64];
    // unfilled (SMM_APPLY_NO_FILL) a padded slot must not see f: it repeats the row's last column, and +0.0 * inf is NaN
    // where the row's own links give -inf.  The planes are finite, as the stacked operator's last column is.
    const bool pad = !fill && k >= len;
    double v[BT][K];
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      const double f = load_fixed(xr[t] + c, fill);
      v[t][0] = pad ? 0.0 : f;
#pragma unroll
      for (int q = 1; q < K; ++q) v[t][q] = load_fixed(gr[t] + (int64_t)(q - 1) * a.g_ld_plane + c, fill);
    }
#pragma unroll
    for (int t = 0; t < BT; ++t) {
#pragma unroll
      for (int q = 0; q < K; ++q) {
        const double p = w[q] * v[t][q];
        acc[t] = acc[t] + p;
      }
    }
  }
  if (len == 0) {   // a row without links never looks at X (its padded slots read column 0)
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[t] = 0.0;
  }
  if (d < a.n_dst) {
    bool dead = false;
    if (a.masked && a.imask) dead = (a.imask[d] == 0);
    if (a.area_min > 0.0 && a.frac) dead = dead || (a.frac[d] < a.area_min);
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      if (j0 + t < a.n_j) yr[t][d] = epilogue(acc[t], dead);
    }
  }
}

int cols_batch_rows(int64_t n_j) { return n_j >= 4 ? 4 : (n_j >= 2 ? 2 : 1); }

// Workgroups of one gather launch of n_j batch rows.  Not monotonic in n_j: three rows take two j-tiles, four take one.
int64_t cols_blocks(int64_t n_dblocks, int64_t n_j) {
  const int bt = cols_batch_rows(n_j);
  return n_dblocks * ((n_j + bt - 1) / bt);
}

int64_t cols_grid_limit() { return std::min<int64_t>(grid_limit(), 0x7fffffffLL); }

template <typename XT, int K>
int launch_cols(ColsArgs a, bool fill, hipStream_t s) {
  auto go = [&](auto bt_tag) -> int {
    constexpr int BT = decltype(bt_tag)::value;
    a.n_jtiles = (a.n_j + BT - 1) / BT;
    const int64_t total = a.n_dblocks * a.n_jtiles;
    if (total <= 0) return SMM_OK;
    if (total > cols_grid_limit())   // the rounds are planned to fit: a slip there is a status, not a launch
      return fail(SMM_ERR_INVALID, "a gather launch of " + std::to_string(a.n_j) + " batch rows needs " + std::to_string(total) +
                                       " workgroups, beyond the launch grid of " + std::to_string(cols_grid_limit()));
    hipLaunchKernelGGL((smm_apply_cols_kernel<XT, K, BT>), dim3((unsigned)total), dim3(kThreads), 0, s, a, fill);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
  };
  switch (cols_batch_rows(a.n_j)) {
    case 4: return go(std::integral_constant<int, 4>());
    case 2: return go(std::integral_constant<int, 2>());
    default: return go(std::integral_constant<int, 1>());
  }
}

template <typename XT>
int launch_cols_k(int n_cols, const ColsArgs& a, bool fill, hipStream_t s) {
  switch (n_cols) {
    case 2: return launch_cols<XT, 2>(a, fill, s);
    case 3: return launch_cols<XT, 3>(a, fill, s);
    default: return launch_cols<XT, 4>(a, fill, s);
  }
}

// The planes of rows [0, n_batch) of x into g; the grid is cut along the batch when it would exceed the launch limit.
int launch_gradients(const smm_grad_plan* plan, const void* x, int x_dtype, int64_t ldx, double* g, int64_t ld_plane,
                     int64_t ld_row, int64_t n_batch, hipStream_t s) {
  GradArgs a{};
  a.si = plan->d_si.get();
  a.sj = plan->d_sj.get();
  a.ci = plan->d_ci.get();
  a.ldx = ldx;
  a.ld_plane = ld_plane;
  a.ld_row = ld_row;
  a.nx = (int)plan->nx;
  a.ny = (int)plan->ny;
  a.periodic = plan->periodic;
  a.n_planes = plan->n_planes;
  for (int p = 0; p < kGradMaxPlanes; ++p) a.kind[p] = plan->kind[p];
  a.n_xtiles = (int)((plan->nx + kGradTileX - 1) / kGradTileX);
  a.n_bands = (int)((plan->ny + kGradBandRows - 1) / kGradBandRows);
  const int64_t per_row = (int64_t)a.n_xtiles * a.n_bands;
  const int64_t limit = std::min<int64_t>(grid_limit(), 0x7fffffffLL);
  if (per_row > limit)
    return fail(SMM_ERR_INVALID, "one batch row alone needs a launch grid beyond " + std::to_string(limit) + " workgroups");
  const int64_t rows_max = limit / per_row;
  const size_t xsz = x_dtype == SMM_F64 ? 8 : 4;
  for (int64_t r0 = 0; r0 < n_batch; r0 += rows_max) {
    const int64_t nr = std::min(rows_max, n_batch - r0);
    a.x = (const char*)x + (size_t)(r0 * ldx) * xsz;
    a.g = g + r0 * ld_row;
    const dim3 grid((unsigned)(nr * per_row));
    if (x_dtype == SMM_F64)
      hipLaunchKernelGGL(smm_gradients_kernel<double>, grid, dim3(kGradTileX), 0, s, a);
    else
      hipLaunchKernelGGL(smm_gradients_kernel<float>, grid, dim3(kGradTileX), 0, s, a);
    SMM_HIP(hipGetLastError());
  }
  return SMM_OK;
}

int check_grad_dtype(int x_dtype) {
  if (x_dtype == SMM_F32 || x_dtype == SMM_F64) return SMM_OK;
  if (x_dtype == SMM_I16 || x_dtype == SMM_U16)
    return fail(SMM_ERR_UNSUPPORTED, "gradients are not built for packed fields (SMM_I16 / SMM_U16): decode the field first");
  if (x_dtype == SMM_F16 || x_dtype == SMM_BF16)
    return fail(SMM_ERR_UNSUPPORTED, "gradients are not built for half-precision fields (SMM_F16 / SMM_BF16)");
  return fail(SMM_ERR_UNSUPPORTED, "field dtype must be SMM_F32 or SMM_F64");
}

}  // namespace

extern "C" {

int smm_grad_plan_create(int64_t nx, int64_t ny, int periodic, int n_planes, const int* plane_kind, const double* si,
                         const double* sj, const double* ci, int device, smm_grad_plan_t* out) {
  return guarded([&]() -> int {
    if (!out) return fail(SMM_ERR_INVALID, "null out handle");
    *out = nullptr;
    if (nx < 1 || ny < 1) return fail(SMM_ERR_INVALID, "nx and ny must be at least 1");
    if (nx > INT32_MAX || ny > INT32_MAX || nx * ny > INT32_MAX)
      return fail(SMM_ERR_INVALID, "nx * ny beyond int32 addressing (SCRIP addresses are int32)");
    if (n_planes < 1 || n_planes > kGradMaxPlanes)
      return fail(SMM_ERR_INVALID, "n_planes=" + std::to_string(n_planes) + " outside 1.." + std::to_string(kGradMaxPlanes));
    if (!plane_kind || !si || !sj || !ci) return fail(SMM_ERR_INVALID, "null table (plane_kind, si, sj, ci)");
    bool has_j = false, has_ij = false;
    for (int p = 0; p < n_planes; ++p) {
      if (plane_kind[p] != SMM_GRAD_I && plane_kind[p] != SMM_GRAD_J && plane_kind[p] != SMM_GRAD_IJ)
        return fail(SMM_ERR_INVALID, "plane_kind[" + std::to_string(p) + "]=" + std::to_string(plane_kind[p]) + " is no SMM_GRAD_* kind");
      has_j = has_j || plane_kind[p] == SMM_GRAD_J;
      has_ij = has_ij || plane_kind[p] == SMM_GRAD_IJ;
    }
    if (has_ij && !has_j) return fail(SMM_ERR_INVALID, "an IJ plane needs a J plane: the cross term differences it");
    int ndev = 0;
    {
      hipError_t e = hipGetDeviceCount(&ndev);
      if (e != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(SMM_ERR_NO_DEVICE, "no HIP device: libsmmregrid_hip has no CPU fallback (hipGetDeviceCount: " +
                                           std::string(hipGetErrorString(e)) + ")");
      }
    }
    if (device < 0 || device >= ndev) return fail(SMM_ERR_NO_DEVICE, "device ordinal " + std::to_string(device) + " out of range");
    std::unique_ptr<smm_grad_plan> plan(new smm_grad_plan());
    plan->device = device;
    plan->nx = nx;
    plan->ny = ny;
    plan->periodic = periodic ? 1 : 0;
    plan->n_planes = n_planes;
    for (int p = 0; p < n_planes; ++p) plan->kind[p] = plane_kind[p];
    DeviceGuard guard(device);
    if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select device " + std::to_string(device));
    SMM_HIP(plan->d_si.upload(std::vector<double>(si, si + 3 * nx)));
    SMM_HIP(plan->d_sj.upload(std::vector<double>(sj, sj + 3 * ny)));
    SMM_HIP(plan->d_ci.upload(std::vector<double>(ci, ci + ny)));
    *out = plan.release();
    return SMM_OK;
  });
}

int smm_grad_plan_destroy(smm_grad_plan_t plan) {
  if (!plan) return SMM_OK;
  DeviceGuard guard(plan->device);
  delete plan;   // also when the device could not be selected
  return SMM_OK;
}

int smm_gradients(smm_grad_plan_t plan, const void* x, int x_dtype, int64_t ldx, double* g, int64_t ld_plane,
                  int64_t ld_row, int64_t n_batch, void* stream) {
  return guarded([&]() -> int {
    if (int rc = check_grad_dtype(x_dtype)) return rc;
    if (!plan) return fail(SMM_ERR_INVALID, "null gradient plan");
    if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
    const int64_t S = plan->nx * plan->ny;
    if (n_batch > 0 && (ldx < S || ld_plane < S || ld_row < (plan->n_planes - 1) * ld_plane + S))
      return fail(SMM_ERR_INVALID, "ldx / ld_plane / ld_row smaller than the grid size");
    if (n_batch == 0) return SMM_OK;
    if (!x || !g) return fail(SMM_ERR_INVALID, "null field pointer");
    if ((uintptr_t)x % (x_dtype == SMM_F64 ? 8 : 4) || (uintptr_t)g % 8)
      return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    DeviceGuard guard(plan->device);
    if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the plan's device");
    return launch_gradients(plan, x, x_dtype, ldx, g, ld_plane, ld_row, n_batch, (hipStream_t)stream);
  });
}

int smm_apply_cols_scratch(smm_operator_t op, int64_t n_batch, size_t* bytes) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (!bytes) return fail(SMM_ERR_INVALID, "null output");
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (op->n_cols < 2)
    return fail(SMM_ERR_INVALID, "the operator has one weight column: smm_operator_create_cols with 2..4 makes the others");
  *bytes = (size_t)n_batch * (size_t)(op->n_cols - 1) * (size_t)op->csr.n_src * sizeof(double);
  return SMM_OK;
}

int smm_apply_cols(smm_operator_t op, smm_grad_plan_t plan, const void* x, int x_dtype, int64_t ldx, void* y,
                   int y_dtype, int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, void* scratch,
                   size_t scratch_bytes, void* stream) {
  return guarded([&]() -> int {
    // what is not built, before the handles are looked at
    if (int rc = check_flags(flags)) return rc;
    if (flags & SMM_APPLY_SKIPNA)
      return fail(SMM_ERR_UNSUPPORTED, "SMM_APPLY_SKIPNA is not built for the K-column apply: a gradient has no valid fraction to renormalise by");
    if (flags & SMM_APPLY_KERNEL_TILE)
      return fail(SMM_ERR_UNSUPPORTED, "the LDS tile kernel is not built for the K-column apply: the gather is the SELL kernel");
    if (flags & (SMM_APPLY_SB_PACKED | SMM_APPLY_SB_Y_SB | SMM_APPLY_HOST_NO_PACK))
      return fail(SMM_ERR_UNSUPPORTED, "the batch-fastest and host-pack flags do not go with the K-column apply: it takes the native (B, S) layout on the device");
    if (int rc = check_grad_dtype(x_dtype)) return rc;
    if (y_dtype != SMM_F64)
      return fail(SMM_ERR_UNSUPPORTED, "the K-column apply produces SMM_F64 results (packed, half and SMM_F32 results are not built)");
    if (!op) return fail(SMM_ERR_INVALID, "null operator");
    if (!plan) return fail(SMM_ERR_INVALID, "null gradient plan");
    if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
    if (op->n_cols < 2)
      return fail(SMM_ERR_INVALID, "the operator has one weight column: smm_operator_create_cols with 2..4 makes the others");
    if (plan->n_planes != op->n_cols - 1)
      return fail(SMM_ERR_INVALID, "the plan has " + std::to_string(plan->n_planes) + " planes, the operator " +
                                       std::to_string(op->n_cols) + " weight columns: one plane per column after the first");
    const int64_t S = op->csr.n_src, D = op->csr.n_dst;
    if (plan->nx * plan->ny != S)
      return fail(SMM_ERR_INVALID, "the plan's grid has " + std::to_string(plan->nx * plan->ny) + " cells, the operator " +
                                       std::to_string(S) + " source cells");
    if (plan->device != op->device) return fail(SMM_ERR_INVALID, "the plan and the operator live on different devices");
    if (n_batch > 0 && (ldx < S || ldy < D)) return fail(SMM_ERR_INVALID, "ldx/ldy smaller than the grid size");
    if (int rc = check_area_min(remap_area_min)) return rc;
    if (int rc = check_epilogue(op, flags & SMM_APPLY_MASKED, remap_area_min, "the operator")) return rc;
    if (n_batch == 0 || D == 0) return SMM_OK;
    if (!x || !y) return fail(SMM_ERR_INVALID, "null field pointer");
    const size_t xsz = x_dtype == SMM_F64 ? 8 : 4;
    if ((uintptr_t)x % xsz || (uintptr_t)y % 8) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    const int n_planes = plan->n_planes;
    const size_t per_row = (size_t)n_planes * (size_t)S * sizeof(double);
    if (!scratch || (uintptr_t)scratch % 8) return fail(SMM_ERR_INVALID, "scratch must be 8-byte aligned device memory");
    if (scratch_bytes < per_row)
      return fail(SMM_ERR_INVALID, "scratch holds " + std::to_string(scratch_bytes) + " bytes, the planes of one batch row need " +
                                       std::to_string(per_row));
    DeviceGuard guard(op->device);
    if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
    hipStream_t s = (hipStream_t)stream;

    ColsArgs a{};
    a.slice_off = op->d_slice_off.get();
    a.col = op->d_col.get();
    a.val = op->d_val.get();
    a.xval = op->d_xval.get();
    a.rowlen = op->d_rowlen.get();
    a.imask = op->d_imask.get();
    a.frac = op->d_frac.get();
    a.g = (const double*)scratch;
    a.n_slots = op->n_slots;
    a.ldx = ldx;
    a.g_ld_plane = S;
    a.g_ld_row = (int64_t)n_planes * S;
    a.ldy = ldy;
    a.n_dst = D;
    a.n_dblocks = ((D + 63) / 64 + kWavesPerBlock - 1) / kWavesPerBlock;
    a.area_min = remap_area_min;
    a.masked = (flags & SMM_APPLY_MASKED) ? 1 : 0;
    const bool fill = !(flags & SMM_APPLY_NO_FILL);
    const int64_t limit = cols_grid_limit();
    if (a.n_dblocks > limit)
      return fail(SMM_ERR_INVALID, "one batch row alone needs a launch grid beyond " + std::to_string(limit) + " workgroups");
    // rows per round: what the scratch holds, and what one gather launch may carry -- the full rounds and the shorter
    // last one, which may block fewer batch rows per thread and so need the larger grid
    int64_t rows = (int64_t)std::min<size_t>(scratch_bytes / per_row, (size_t)n_batch);
    auto fits = [&](int64_t r) {
      const int64_t tail = n_batch % r;
      return cols_blocks(a.n_dblocks, r) <= limit && (tail == 0 || cols_blocks(a.n_dblocks, tail) <= limit);
    };
    while (rows > 1 && !fits(rows)) rows = (rows + 1) / 2;
    for (int64_t r0 = 0; r0 < n_batch; r0 += rows) {
      const int64_t nr = std::min(rows, n_batch - r0);
      const char* xr = (const char*)x + (size_t)(r0 * ldx) * xsz;
      if (int rc = launch_gradients(plan, xr, x_dtype, ldx, (double*)scratch, a.g_ld_plane, a.g_ld_row, nr, s)) return rc;
      a.x = xr;
      a.y = (double*)y + r0 * ldy;
      a.n_j = nr;
      const int rc = x_dtype == SMM_F64 ? launch_cols_k<double>(op->n_cols, a, fill, s) : launch_cols_k<float>(op->n_cols, a, fill, s);
      if (rc) return rc;
    }
    return SMM_OK;
  });
}

}  // extern "C"
