// Device-side element helpers of the convolution family and the kernels around it (gconv.hip, wgrad.hip, wpack.hip, convaux.hip,
// norm.hip, loss.hip, wfold.hip, timed.hip and the dedicated single-layer files): the 16-bit storage type and its vectors, elements
// per 16-byte piece, conversions, the reflect index, the activations.  Everything here has internal linkage: every translation
// unit gets its own copy, exactly as when each file spelled them out.
#pragma once
#include "common.h"

namespace {

typedef p2phd_h16 bf16_t;                 // the library's 16-bit storage type: bf16, or fp16 in the -DP2PHD_F16 build (common.h)

template <typename T> struct Elem;
template <> struct Elem<float> { static constexpr int EPP = 4; };    // elements per 16-byte piece
template <> struct Elem<bf16_t> { static constexpr int EPP = 8; };

constexpr int kRowBytes = 128;   // bytes of K per LDS tile row

#ifdef __HIPCC__
typedef __attribute__((ext_vector_type(8))) bf16_t bf16x8;
typedef __attribute__((ext_vector_type(4))) bf16_t bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float v) { return (bf16_t)v; }

__device__ __forceinline__ int reflect_idx(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case P2PHD_ACT_LRELU: return v > 0.f ? v : 0.2f * v;
    case P2PHD_ACT_TANH: return tanhf(v);
    case P2PHD_ACT_RELU: return v > 0.f ? v : 0.f;
    default: return v;
  }
}
#endif

}  // namespace

// host launchers of kernels that exist for the 16-bit type and for f32: run `...` with T naming the element type of `dtype`
#define FOR_ELEM(dtype, T, ...) do { if ((dtype) == P2PHD_BF16) { typedef bf16_t T; __VA_ARGS__; } else { typedef float T; __VA_ARGS__; } } while (0)
