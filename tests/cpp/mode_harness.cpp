// The row rule of the categorical apply (smmregrid_amd/csrc/smm_mode.hpp: mode_row, the function both forms of
// smm_mode_kernel run) on the CPU, for tests/test_mode_harness.py: built with the host compiler under AddressSanitizer +
// UBSan, fed the cases of tests/mode_cases.py, compared with categorical.ModeRule bit for bit.
//
//   mode_harness <in> <out>
// in:  int64 n_dst, n_src, n_batch, ldx, dtype (SMM_F32 0, SMM_F64 1, SMM_I16 2, SMM_U16 3), n_fill, fill0, fill1,
//      fill_out, masked; double area_min; int64 rowptr[n_dst + 1]; int32 col[nnz]; double val[nnz]; uint8 imask[n_dst];
//      double frac[n_dst]; the field x[n_batch * ldx] of its own type
// out: y[n_batch * n_dst] of the field's type, then double share[n_batch * n_dst]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_mode.hpp"

namespace {

template <typename T>
std::vector<T> read_vec(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

template <typename XT, typename CT>
struct CsrLinks {
  const XT* row;
  const int32_t* col;
  const double* w;
  CT value(int k) const { return (CT)row[col[k]]; }
  double weight(int k) const { return w[k]; }
};

template <typename XT, typename CT>
int run(FILE* in, FILE* out, const int64_t* h, double area_min, const std::vector<int64_t>& rowptr,
        const std::vector<int32_t>& col, const std::vector<double>& val, const std::vector<uint8_t>& imask,
        const std::vector<double>& frac) {
  const int64_t D = h[0], B = h[2], ldx = h[3];
  const std::vector<XT> x = read_vec<XT>(in, (size_t)(B * ldx));
  ModeMissing miss;
  miss.n_fill = (int32_t)h[5];
  miss.fill[0] = (int32_t)h[6];
  miss.fill[1] = (int32_t)h[7];
  std::vector<XT> y((size_t)(B * D));
  std::vector<double> share((size_t)(B * D));
  for (int64_t b = 0; b < B; ++b)
    for (int64_t d = 0; d < D; ++d) {
      const int64_t lo = rowptr[d];
      const CsrLinks<XT, CT> links{x.data() + b * ldx, col.data() + lo, val.data() + lo};
      const ModeResult r = mode_row((int)(rowptr[d + 1] - lo), links, miss, h[9] != 0 && imask[d] == 0, frac[d], area_min);
      XT v;
      if (r.k >= 0) v = (XT)links.value(r.k);
      else if constexpr (std::is_integral<XT>::value) v = (XT)h[8];
      else v = (XT)NAN;
      y[(size_t)(b * D + d)] = v;
      share[(size_t)(b * D + d)] = r.share;
    }
  fwrite(y.data(), sizeof(XT), y.size(), out);
  fwrite(share.data(), sizeof(double), share.size(), out);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const std::vector<int64_t> h = read_vec<int64_t>(in, 10);
  const double area_min = read_vec<double>(in, 1)[0];
  const int64_t D = h[0];
  const auto rowptr = read_vec<int64_t>(in, (size_t)D + 1);
  const size_t nnz = (size_t)rowptr[(size_t)D];
  const auto col = read_vec<int32_t>(in, nnz);
  const auto val = read_vec<double>(in, nnz);
  const auto imask = read_vec<uint8_t>(in, (size_t)D);
  const auto frac = read_vec<double>(in, (size_t)D);
  int rc = 2;
  switch (h[4]) {
    case 0: rc = run<float, float>(in, out, h.data(), area_min, rowptr, col, val, imask, frac); break;
    case 1: rc = run<double, double>(in, out, h.data(), area_min, rowptr, col, val, imask, frac); break;
    case 2: rc = run<int16_t, int32_t>(in, out, h.data(), area_min, rowptr, col, val, imask, frac); break;
    case 3: rc = run<uint16_t, int32_t>(in, out, h.data(), area_min, rowptr, col, val, imask, frac); break;
  }
  fclose(in);
  fclose(out);
  return rc;
}
