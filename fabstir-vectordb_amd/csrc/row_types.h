// row_types.h — the element type of a stored row: float (f32 rows) or half_t (IEEE binary16 rows).
// A kernel that reads stored rows is a template over it; everything it does with a row happens in f32, and the only
// things that differ are the load and the widen.  Widening binary16 -> f32 is exact (every half, subnormals and
// infinities included, is an f32), so a half row scored here is the f32 row holding the same values, bit for bit.
#pragma once
#include "common.h"

namespace fvdb {

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

// Pair: dims (2l, 2l+1) of a row as one lane loads them; Quad: four consecutive dims.  Row strides are multiples of
// four elements, so a Pair is 4-byte and a Quad 8-byte aligned whatever the element.
template <typename RT>
struct RowVec;
template <>
struct RowVec<float> {
  using Pair = float2;
  using Quad = float4;
  static __device__ __forceinline__ Pair zero_pair() { return make_float2(0.0f, 0.0f); }
};
template <>
struct RowVec<half_t> {
  using Pair = half2_t;
  using Quad = half4_t;
  static __device__ __forceinline__ Pair zero_pair() { return Pair{(half_t)0.0f, (half_t)0.0f}; }
};

__device__ __forceinline__ float row_widen(float v) { return v; }
__device__ __forceinline__ float row_widen(half_t v) { return (float)v; }
__device__ __forceinline__ float2 row_widen(float2 v) { return v; }
__device__ __forceinline__ float2 row_widen(half2_t v) { return make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ float4 row_widen(float4 v) { return v; }
__device__ __forceinline__ float4 row_widen(half4_t v) { return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w); }

// dims (j, j + 1) of a stored row, widened (j even)
template <typename RT>
__device__ __forceinline__ float2 row_pair_f32(const RT* row, uint32_t j) {
  return row_widen(*(const typename RowVec<RT>::Pair*)(row + j));
}

}  // namespace fvdb
