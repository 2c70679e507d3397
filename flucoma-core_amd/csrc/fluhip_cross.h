// fluhip_cross.h -- launch interface of kernels_nmfcross.hip (BufNMFCross: NMFCross's H update, its constraint stencils,
// the synthesis product and the Griffin-Lim steps).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace fluhip {

enum : int
{
  kCrossEpiStore = 0,   // C = sum
  kCrossEpiRatio = 1,   // C = V / max(sum, eps)
  kCrossEpiHUpdate = 2, // C = (Hc * sum) / max(den[n], eps)
  kCrossEpiPartial = 3  // (internal) the split's raw sums
};

// C[m][n] (row stride ldc) = epilogue(sum_k A(m, k) B(n, k)) over M x N with a contraction of Kd; A row-major M x Kd
// (lda); B row-major N x Kd (TB = 0) or Kd x N (TB = 1), row stride ldb
struct CrossGemm
{
  const double* A;
  int64_t lda;
  const double* B;
  int64_t ldb;
  double* C;
  int64_t ldc;
  int64_t M, N, Kd;
  const double* V = nullptr;  // kCrossEpiRatio: [M][ldv]
  int64_t ldv = 0;
  const double* Hc = nullptr; // kCrossEpiHUpdate: [M][ldh]
  int64_t ldh = 0;
  const double* den = nullptr; // kCrossEpiHUpdate: [N]
  int64_t kChunk = 0, splitStride = 0; // (set by launch_cross_gemm)
};

// tile form and contraction split of one GEMM shape for a device of `cus` compute units
struct CrossGemmPlan
{
  bool big = false; // 128 x 128 workgroup tiles (else 64 x 64)
  int nsplit = 1;
  int64_t kChunk = 0;
  int64_t partDoubles = 0; // workspace the split needs
};
CrossGemmPlan cross_gemm_plan(int64_t M, int64_t N, int64_t Kd, int cus);
// tb: layout of B as above; A is always row-major M x Kd
void launch_cross_gemm(CrossGemm g, int ta, int tb, int epi, const CrossGemmPlan& p, double* part, hipStream_t s);

void launch_cross_dict(double* W, int64_t ldw, int K, int F, double* colsum, double* energy, hipStream_t s);
void launch_cross_continuity(const double* H, double* Hc, int64_t ldh, int T, int K, int c, hipStream_t s);
void launch_cross_sparsity(const double* H, double* out, int64_t ldh, int T, int K, int r, hipStream_t s);
void launch_cross_polyphony(double* H, int64_t ldh, int T, int K, const double* energy, int p, hipStream_t s);

void launch_gl_apply(const double* mag, const double* phase, double* spec, int64_t n, hipStream_t s);
void launch_gl_update(const double* mag, const double* est, const double* prev, double* spec, int64_t n, hipStream_t s);

} // namespace fluhip
