// Host-only harness around the weight-column builder of smm_build.cpp (build_csr_cols, prune_zero_links_cols,
// build_sell_cols: what smm_operator_create_cols runs before anything is uploaded), compiled with
// g++ -fsanitize=address,undefined by tests/test_build_cols.py.
// argv[1]: host threads of the builders (0 / absent = automatic)
// stdin : n_src n_dst nnz n_cols prune, then nnz lines "src1 dst1 w0 .. w(n_cols-1)"
// stdout: ERROR <text> when the builder refuses; else
//   CSR <nnz>, the rowptr line, the col line, one "VAL <k>" line per column of the canonical CSR,
//   COL0BAD <n>    differences between column 0 and build_csr's output on that column alone (bits compared),
//   SELLBAD <n>    slots of the extra columns' SELL planes that differ from the CSR, padded slots that are not +0.0,
//   with prune != 0: PRUNED <dropped> <nnz>, then the col line and the VAL lines of the pruned matrix.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_internal.h"

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

static void print_matrix(const smm::HostCsr& csr, const std::vector<std::vector<double>>& extra) {
  for (int64_t p = 0; p < csr.nnz; ++p) printf("%d ", csr.col[(size_t)p]);
  printf("\n");
  for (size_t k = 0; k <= extra.size(); ++k) {
    printf("VAL %zu ", k);
    for (int64_t p = 0; p < csr.nnz; ++p) printf("%.17g ", k == 0 ? csr.val[(size_t)p] : extra[k - 1][(size_t)p]);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc > 1) smm::set_host_threads(atoi(argv[1]));
  long long n_src, n_dst, nnz;
  int n_cols, prune;
  if (scanf("%lld %lld %lld %d %d", &n_src, &n_dst, &nnz, &n_cols, &prune) != 5) return 2;
  const int width = n_cols > 0 ? n_cols : 1;   // the lines carry at least one weight
  std::vector<int32_t> src((size_t)nnz), dst((size_t)nnz);
  std::vector<double> w((size_t)nnz * (size_t)width);
  for (long long k = 0; k < nnz; ++k) {
    if (scanf("%d %d", &src[(size_t)k], &dst[(size_t)k]) != 2) return 2;
    for (int c = 0; c < width; ++c)
      if (scanf("%lf", &w[(size_t)k * (size_t)width + (size_t)c]) != 1) return 2;
  }
  smm::HostCsr csr;
  std::vector<std::vector<double>> extra;
  std::string err;
  if (!smm::build_csr_cols(n_src, n_dst, nnz, src.data(), dst.data(), w.data(), n_cols, csr, extra, err)) {
    printf("ERROR %s\n", err.c_str());
    return 0;
  }
  printf("CSR %lld\n", (long long)csr.nnz);
  for (int64_t d = 0; d <= csr.n_dst; ++d) printf("%lld ", (long long)csr.rowptr[(size_t)d]);
  printf("\n");
  print_matrix(csr, extra);

  // column 0 is the one-column builder's output, bit for bit
  long long bad0 = (long long)extra.size() != n_cols - 1;
  {
    std::vector<double> w0((size_t)nnz);
    for (long long k = 0; k < nnz; ++k) w0[(size_t)k] = w[(size_t)k * (size_t)width];
    smm::HostCsr one;
    std::string err1;
    if (!smm::build_csr(n_src, n_dst, nnz, src.data(), dst.data(), w0.data(), one, err1)) ++bad0;
    if (one.nnz != csr.nnz || one.rowptr != csr.rowptr || one.col != csr.col || one.n_used_src != csr.n_used_src ||
        one.max_row_nnz != csr.max_row_nnz)
      ++bad0;
    else
      for (int64_t p = 0; p < csr.nnz; ++p) bad0 += !same_bits(one.val[(size_t)p], csr.val[(size_t)p]);
    for (const std::vector<double>& e : extra) bad0 += (int64_t)e.size() != csr.nnz;
  }
  printf("COL0BAD %lld\n", bad0);

  // the SELL planes of the extra columns follow build_sell's slots; padding is +0.0
  smm::HostSell sell;
  smm::build_sell(csr, sell);
  std::vector<double> planes;
  smm::build_sell_cols(csr, sell, extra, planes);
  long long sbad = (int64_t)planes.size() != sell.n_slots * (int64_t)extra.size();
  if (!sbad) {
    for (size_t k = 0; k < extra.size(); ++k) {
      const double* plane = planes.data() + k * (size_t)sell.n_slots;
      for (int64_t s = 0; s < sell.n_slices; ++s) {
        const int64_t nslots = (sell.slice_off[(size_t)s + 1] - sell.slice_off[(size_t)s]) / 64;
        for (int64_t r = 0; r < 64; ++r) {
          const int64_t d = s * 64 + r;
          const int64_t len = d < csr.n_dst ? csr.rowptr[(size_t)d + 1] - csr.rowptr[(size_t)d] : 0;
          for (int64_t i = 0; i < nslots; ++i) {
            const double v = plane[(size_t)(sell.slice_off[(size_t)s] + r + i * 64)];
            if (i < len)
              sbad += !same_bits(v, extra[k][(size_t)(csr.rowptr[(size_t)d] + i)]);
            else
              sbad += !(v == 0.0 && !std::signbit(v));
          }
        }
      }
    }
  }
  printf("SELLBAD %lld\n", sbad);

  if (prune) {
    const int64_t dropped = smm::prune_zero_links_cols(csr, extra);
    printf("PRUNED %lld %lld\n", (long long)dropped, (long long)csr.nnz);
    for (int64_t d = 0; d <= csr.n_dst; ++d) printf("%lld ", (long long)csr.rowptr[(size_t)d]);
    printf("\n");
    print_matrix(csr, extra);
  }
  return 0;
}
