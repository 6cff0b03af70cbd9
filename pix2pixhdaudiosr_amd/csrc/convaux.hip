// Small kernels around a gather-convolution launch (gconv.hip): the expanded gradient and the fold of reflect-padded input
// gradients, the bias gradient, the merge of the fused InstanceNorm-backward sums.
#include "common.h"
#include "convplan.h"
#include "convdev.h"

namespace {

// E[n, r', c', :] for the pad_mode 2 gather (see gconv_kernel): rows r' < H are dy's, r' = H holds dy[0] + dy[2],
// r' = H + 1 holds dy[H-3] + dy[H-1]; the same along W (corners: sums of sums).  H, W >= 3.
template <typename T>
__global__ void reflect_expand_kernel(const T* __restrict__ dy, T* __restrict__ e_out, int N, int H, int W, int Cp) {
  constexpr int EPP = Elem<T>::EPP;
  const int cpr = Cp / EPP;
  const int He = H + 2, We = W + 2;
  const long total = (long)N * He * We * cpr;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int pc = (int)(e % cpr);
    long r = e / cpr;
    const int j = (int)(r % We); r /= We;
    const int i = (int)(r % He);
    const int n = (int)(r / He);
    int hs[2], ws[2], nh = 1, nw = 1;
    hs[0] = i; ws[0] = j;
    if (i == H) { hs[0] = 0; hs[nh++] = 2; } else if (i == H + 1) { hs[0] = H - 3; hs[nh++] = H - 1; }
    if (j == W) { ws[0] = 0; ws[nw++] = 2; } else if (j == W + 1) { ws[0] = W - 3; ws[nw++] = W - 1; }
    uint4 ov;
    if (nh == 1 && nw == 1) {
      ov = *reinterpret_cast<const uint4*>(dy + (((size_t)n * H + hs[0]) * W + ws[0]) * Cp + pc * EPP);
    } else {
      float acc[EPP];
#pragma unroll
      for (int k = 0; k < EPP; ++k) acc[k] = 0.f;
      for (int a = 0; a < nh; ++a)
        for (int b = 0; b < nw; ++b) {
          const uint4 v = *reinterpret_cast<const uint4*>(dy + (((size_t)n * H + hs[a]) * W + ws[b]) * Cp + pc * EPP);
          const T* vv = reinterpret_cast<const T*>(&v);
#pragma unroll
          for (int k = 0; k < EPP; ++k) acc[k] += to_f(vv[k]);
        }
      T* oo = reinterpret_cast<T*>(&ov);
#pragma unroll
      for (int k = 0; k < EPP; ++k) oo[k] = from_f<T>(acc[k]);
    }
    *reinterpret_cast<uint4*>(e_out + (size_t)e * EPP) = ov;
  }
}

// reflect-pad adjoint: dx[n,i,j,:] = sum over padded positions that mirror onto (i,j) of dxp (+ addend)
template <typename T>
__global__ void reflect_fold_kernel(const T* __restrict__ dxp, const T* __restrict__ addend, T* __restrict__ dx,
                                    int N, int H, int W, int Cp, int P) {
  constexpr int EPP = Elem<T>::EPP;
  const int cpr = Cp / EPP;
  const long total = (long)N * H * W * cpr;
  const int Hp = H + 2 * P, Wp = W + 2 * P;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int pc = (int)(e % cpr);
    long r = e / cpr;
    const int j = (int)(r % W); r /= W;
    const int i = (int)(r % H);
    const int n = (int)(r / H);
    int hs[3], ws[3], nh = 1, nw = 1;                            // a row within P of BOTH borders (H <= 2 P + 1) has two mirrors
    hs[0] = i + P; ws[0] = j + P;
    if (i >= 1 && i <= P) hs[nh++] = P - i;
    if (i >= H - 1 - P && i <= H - 2) hs[nh++] = 2 * (H - 1) - i + P;
    if (j >= 1 && j <= P) ws[nw++] = P - j;
    if (j >= W - 1 - P && j <= W - 2) ws[nw++] = 2 * (W - 1) - j + P;
    float acc[EPP];
#pragma unroll
    for (int k = 0; k < EPP; ++k) acc[k] = 0.f;
    for (int a = 0; a < nh; ++a)
      for (int b = 0; b < nw; ++b) {
        const uint4 v = *reinterpret_cast<const uint4*>(dxp + (((size_t)n * Hp + hs[a]) * Wp + ws[b]) * Cp + pc * EPP);
        const T* vv = reinterpret_cast<const T*>(&v);
#pragma unroll
        for (int k = 0; k < EPP; ++k) acc[k] += to_f(vv[k]);
      }
    const size_t o = (((size_t)n * H + i) * W + j) * Cp + pc * EPP;
    if (addend != nullptr) {
      const uint4 v = *reinterpret_cast<const uint4*>(addend + o);
      const T* vv = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int k = 0; k < EPP; ++k) acc[k] += to_f(vv[k]);
    }
    uint4 ov;
    T* oo = reinterpret_cast<T*>(&ov);
#pragma unroll
    for (int k = 0; k < EPP; ++k) oo[k] = from_f<T>(acc[k]);
    *reinterpret_cast<uint4*>(dx + o) = ov;
  }
}

// column sums of a [P][Cp] matrix (bias gradient): db[c] (+)= sum_p x[p][c].
// Block = cpg channel pieces x R pixel rows; the rows of a block meet in LDS and are added in row order, the blocks of a
// column group store their partial row and the LAST of them (fold_arrive_last) adds the rows in block order: no float
// atomics, the same bits on every run (these are the biases with a real gradient: no InstanceNorm behind the conv).
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, long P, int Cp, int K, float* __restrict__ db, int cpg,
                                                     int accumulate, float* __restrict__ part, unsigned* __restrict__ tickets) {
  constexpr int EPP = Elem<T>::EPP;
  __shared__ float red[256 * 8];
  const int cpr = Cp / EPP;
  const int pl = threadIdx.x % cpg, rl = threadIdx.x / cpg, R = 256 / cpg;
  const int pc = blockIdx.y * cpg + pl;
  float acc[EPP];
#pragma unroll
  for (int k = 0; k < EPP; ++k) acc[k] = 0.f;
  if (pc < cpr) {
    // four rows per trip, all requested before the first is added (one 16-byte load in flight per thread left this pass at
    // 2.7 TB/s); rows past the end re-read the last one and are masked in the sum (no branch around a load)
    constexpr int U = 4;
    const long stride = (long)gridDim.x * R;
    for (long p0 = (long)blockIdx.x * R + rl; p0 < P; p0 += stride * U) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long p = p0 + stride * u;
        v[u] = *reinterpret_cast<const uint4*>(x + (size_t)(p < P ? p : P - 1) * Cp + pc * EPP);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float live = p0 + stride * u < P ? 1.f : 0.f;
        const T* vv = reinterpret_cast<const T*>(&v[u]);
#pragma unroll
        for (int k = 0; k < EPP; ++k) acc[k] += to_f(vv[k]) * live;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < EPP; ++k) red[threadIdx.x * 8 + k] = acc[k];
  __syncthreads();
  const int width = cpg * EPP;                                   // channels of this column group
  float* rows = part + (size_t)blockIdx.y * gridDim.x * width;
  if (rl == 0) {
#pragma unroll
    for (int k = 0; k < EPP; ++k) {
      float t = 0.f;
      for (int r = 0; r < R; ++r) t += red[(r * cpg + pl) * 8 + k];
      p2phd::fold_store(rows + (size_t)blockIdx.x * width + pl * EPP + k, t);
    }
  }
  if (!p2phd::fold_arrive_last(tickets + blockIdx.y, gridDim.x)) return;
  const int nb = (int)gridDim.x;
  for (int j = threadIdx.x; j < width; j += 256) {
    const int c = blockIdx.y * width + j;
    if (c >= K) continue;
    float s = 0.f;
    for (int b = 0; b < nb; b += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p2phd::fold_load(rows + (size_t)min(b + u, nb - 1) * width + j);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += b + u < nb ? v[u] : 0.f;
    }
    db[c] = accumulate ? db[c] + s : s;
  }
}

// bstats[n][c] = sum over tiles (and sub-pixel classes) of the partials one input-gradient launch left (GDesc::bs_out):
// one wavefront per (sample, channel), lanes over tiles, fixed shuffle tree -> the result does not depend on timing.
// Pad channels [C, Cp) are written as zeros here (they used to cost a memset node per launch).
__global__ __launch_bounds__(256) void bsum_merge_kernel(const float* __restrict__ part, float* __restrict__ bstats, int tiles,
                                                         int n_extent, int cls_cp, int Cp, int C) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
  if (c >= Cp) return;
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const int ncls = cls_cp > 0 ? 4 : 1;
    for (int t = lane; t < tiles; t += 64)
      for (int q = 0; q < ncls; ++q) {
        const float2 v = *reinterpret_cast<const float2*>(part + (((size_t)n * tiles + t) * n_extent + q * cls_cp + c) * 2);
        s1 += v.x; s2 += v.y;
      }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
  }
  if (lane == 0) *reinterpret_cast<float2*>(bstats + 2 * ((size_t)n * Cp + c)) = make_float2(s1, s2);
}

}  // namespace

namespace p2phd {

int launch_bsum_merge(const float* table, float* bstats, int N, long npix, int tile_rows, int n_extent, int cls_cp, int Cp, int C,
                      hipStream_t st) {
  const int tiles = (int)((npix + tile_rows - 1) / tile_rows);
  hipLaunchKernelGGL(bsum_merge_kernel, dim3((unsigned)((Cp + 3) / 4), (unsigned)N), dim3(256), 0, st, table, bstats, tiles, n_extent,
                     cls_cp, Cp, C);
  return check_launch("bsum_merge");
}

int launch_reflect_fold(int dtype, const void* dxp, const void* addend, void* dx, int N, int H, int W, int Cp, int P,
                        hipStream_t st) {
  const int epp = dtype == P2PHD_BF16 ? 8 : 4;
  const long total = (long)N * H * W * (Cp / epp);
  const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
  FOR_ELEM(dtype, T, hipLaunchKernelGGL(reflect_fold_kernel<T>, dim3(blocks), dim3(256), 0, st, (const T*)dxp, (const T*)addend, (T*)dx, N, H, W, Cp, P));
  return check_launch("reflect_fold");
}

int launch_reflect_expand(int dtype, const void* dy, void* e_out, int N, int H, int W, int Cp, hipStream_t st) {
  const int epp = dtype == P2PHD_BF16 ? 8 : 4;
  const long total = (long)N * (H + 2) * (W + 2) * (Cp / epp);
  const int blocks = (int)std::min<long>((total + 255) / 256, 8192);
  FOR_ELEM(dtype, T, hipLaunchKernelGGL(reflect_expand_kernel<T>, dim3(blocks), dim3(256), 0, st, (const T*)dy, (T*)e_out, N, H, W, Cp));
  return check_launch("reflect_expand");
}

int launch_colsum(int dtype, const void* x, long P, int Cp, int K, float* db, int accumulate, hipStream_t st) {
  if (P == 0) {
    if (!accumulate) (void)hipMemsetAsync(db, 0, sizeof(float) * (size_t)K, st);
    return P2PHD_OK;
  }
  const int epp = dtype == P2PHD_BF16 ? 8 : 4;
  const int cpr = Cp / epp;
  int cpg = 1;
  while (cpg * 2 <= cpr && cpg * 2 <= 64) cpg *= 2;
  const int R = 256 / cpg;
  const int ygroups = (cpr + cpg - 1) / cpg;
  const FoldScratch fs = fold_scratch(FOLD_COLSUM, st);
  if (fs.part == nullptr) return P2PHD_EINVAL;                   // (refused: error text set by fold_scratch)
  P2PHD_REQUIRE(ygroups <= fs.tickets, "colsum: too many channels (%d)", Cp);
  const long rows_max = (long)(fs.floats / ((size_t)ygroups * cpg * epp));   // partial rows per column group
  P2PHD_REQUIRE(rows_max >= 1, "colsum: too many channels for the reduction scratch");
  const int xblocks = (int)std::max<long>(1, std::min<long>(std::min<long>((P + R * 32 - 1) / (R * 32), 512), rows_max));
  dim3 grid(xblocks, ygroups);
  FOR_ELEM(dtype, T, hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, st, (const T*)x, P, Cp, K, db, cpg, accumulate, fs.part, fs.ticket));
  return check_launch("colsum");
}

}  // namespace p2phd
