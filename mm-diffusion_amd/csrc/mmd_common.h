// Shared device/host helpers for libmmd (gfx950 / CDNA4 only - no CUDA compat, no dual paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/mmd.h"   // the C ABI: every extern "C" definition is checked against its declaration

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

// ----------------------------------------------------------------------------- error plumbing
int mmd_set_error(int code, const char* fmt, ...);
int mmd_check_launch(const char* what);

#define MMD_REQUIRE(cond, ...)                                  \
  do {                                                          \
    if (!(cond)) return mmd_set_error(MMD_ERR_ARG, __VA_ARGS__); \
  } while (0)

// ----------------------------------------------------------------------------- bf16 <-> f32
__device__ __forceinline__ float bf16_bits_to_f32(uint32_t bits16) { return __uint_as_float(bits16 << 16); }
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {   // round-to-nearest-even
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;            // NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  return f32_to_bf16_bits(lo) | (f32_to_bf16_bits(hi) << 16);
}

// Element traits: T = float or __bf16.  A "vec" is always 16 bytes.
template <typename T> struct Elt;
template <> struct Elt<float> {
  static constexpr int EPV = 4;      // elements per 16-byte vec
  static constexpr int DT = MMD_F32;
  __device__ static __forceinline__ void unpack(const u32x4& v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(v[i]);
  }
  __device__ static __forceinline__ u32x4 pack(const float* f) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __float_as_uint(f[i]);
    return v;
  }
  __device__ static __forceinline__ float ld(const void* p, int64_t i) { return ((const float*)p)[i]; }
  __device__ static __forceinline__ void st(void* p, int64_t i, float v) { ((float*)p)[i] = v; }
};
template <> struct Elt<__bf16> {
  static constexpr int EPV = 8;
  static constexpr int DT = MMD_BF16;
  __device__ static __forceinline__ void unpack(const u32x4& v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(v[i] << 16);
      f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ u32x4 pack(const float* f) {   // RNE; lowers to v_cvt_pk_bf16_f32
    bf16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (__bf16)f[i];
    return __builtin_bit_cast(u32x4, t);
  }
  __device__ static __forceinline__ float ld(const void* p, int64_t i) {
    return bf16_bits_to_f32(((const uint16_t*)p)[i]);
  }
  __device__ static __forceinline__ void st(void* p, int64_t i, float v) {
    ((__bf16*)p)[i] = (__bf16)v;
  }
};

// SiLU with v_rcp_f32 (1 ulp) instead of an IEEE division: 5 VALU instructions per element where the division sequence took 14.  Every
// kernel that applies SiLU in the forward uses this one function, so fused and unfused paths stay bitwise equal.
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// silu'(v) = sg (1 + v (1 - sg)) with the same v_rcp_f32 sigmoid sg: the IEEE division is ~10 more VALU instructions per element.
__device__ __forceinline__ float dsilu_f(float v) {
  const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-v));
  return sg * (1.f + v * (1.f - sg));
}

// Zeroes DT 32x32 MFMA accumulators
template <int DT>
__device__ __forceinline__ void zero_acc(f32x16 (&o)[DT]) {
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
}

// 64-lane butterfly reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum over the 32 lanes of each half-wave without LDS traffic or selects: four DPP row rotations give every lane of a 16-lane row the
// row total, row_bcast:15 then adds the total of rows 0 / 2 into rows 1 / 3.  Valid in lanes 16-31 (half 0) and 48-63 (half 1).
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, false));
}
__device__ __forceinline__ float halfwave_total(float v) {
  v = dpp_add<0x128, 0xf>(v);      // row_ror:8
  v = dpp_add<0x124, 0xf>(v);      // row_ror:4
  v = dpp_add<0x122, 0xf>(v);      // row_ror:2
  v = dpp_add<0x121, 0xf>(v);      // row_ror:1
  return dpp_add<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
}

// Fixed-order sum over the 256 threads of a block, of any number of LDS arrays at once: the caller has stored its value at s[tid];
// s[tid] += s[tid + o] for o = 128 ... 1, one barrier per level.  On return s[0] holds the total and every thread may read it.  The
// order never depends on the grid, so the per-sample reductions built on it (loss_terms, vlb_terms, dpm_err, sumsq_chunks) are
// bitwise repeatable.
template <class... T>
__device__ __forceinline__ void block_tree_sum256(int tid, T*... s) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) ((s[tid] += s[tid + o]), ...);
    __syncthreads();
  }
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// grid of a 256-thread grid-stride element-wise kernel: one thread per element up to 4096 blocks
static inline int ew_grid(int64_t total) { return (int)min((int64_t)4096, (total + 255) / 256); }

#define MMD_MAX_DEVICES 16
static inline int mmd_device_slot() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d & (MMD_MAX_DEVICES - 1);
}

// ----------------------------------------------------------------------------- launching
// Every kernel of the library is launched here.  mmd_launch_cap<K> raises K's dynamic-LDS limit to `cap` bytes (>= lds) when the launch
// needs more than K has been granted on the current device (everything starts at the 64 KB default), launches, and returns
// mmd_check_launch(what).  The limit is a per-DEVICE property of a kernel, so the granted size is kept per kernel and device slot: a
// running maximum, hence a launch sequence that has run once makes no attribute call when it is repeated (under graph capture, say).
// With the switch values read once and the read-only zero pages this is all the process-lifetime state of the library; a benign race
// sets a limit twice.
template <auto K, class... A>
static int mmd_launch_cap(const char* what, dim3 grid, dim3 block, size_t lds, size_t cap, hipStream_t st, const A&... args) {
  if (lds > 64 * 1024) {
    static size_t granted[MMD_MAX_DEVICES] = {};
    size_t& g = granted[mmd_device_slot()];
    if (lds > g) {
      hipError_t e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
      if (e != hipSuccess) return mmd_set_error(MMD_ERR_LAUNCH, "%s: set LDS attr: %s", what, hipGetErrorString(e));
      g = cap;
    }
  }
  hipLaunchKernelGGL(K, grid, block, lds, st, args...);
  return mmd_check_launch(what);
}
template <auto K, class... A>
static int mmd_launch(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  return mmd_launch_cap<K>(what, grid, block, lds, lds, st, args...);
}

// Calls f with a tag of the element type of `dtype`: [&](auto t) { using T = typename decltype(t)::type; ... }
template <typename T> struct mmd_type { using type = T; };
template <class F>
static int mmd_by_dtype(int dtype, F&& f) { return dtype == MMD_BF16 ? f(mmd_type<__bf16>{}) : f(mmd_type<float>{}); }

// ----------------------------------------------------------------------------- environment switches
int mmd_env_int(const char* name, int dflt);   // the value if it is a positive integer, else dflt
char mmd_env_char(const char* name);           // first character of the value; 0 if unset or empty
bool mmd_env_set(const char* name);            // set at all, to anything
