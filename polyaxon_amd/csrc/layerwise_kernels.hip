// Layer-wise adaptive updates (LARS / LAMB) over the flat parameter buffer on MI355X (gfx950).
//
// Both rules scale each weight tensor's update by a trust ratio built from two L2 norms over that tensor alone, so the
// step needs ~160 segmented norms whose sizes run from under one vector to 38.7 M elements (GPT-2's embedding).  The
// work is cut into fixed-size chunks that never cross a segment (a host-built table, ops/optim.py _Layerwise):
//
//   plx_lw_norms    one workgroup per chunk (grid-strided under a cap): two fp32 sums of squares per chunk into
//                   partials[2c], partials[2c + 1].  LARS: sum w^2, sum g^2.  LAMB: the pass advances the AdamW
//                   moments, stores them, forms u = m^/(sqrt(v^) + eps) + wd w and writes sum w^2, sum u^2.
//   plx_lw_ratios   one wave per segment sums its chunks' partials in chunk order (fp64) and writes ratio[segment].
//   plx_lw_update   one workgroup per chunk reads ratio[segment] once and applies the update; the gradients are zeroed.
//
// Nothing here is atomic and no sum depends on scheduling: a chunk belongs to one workgroup whatever the grid, a lane's
// elements and their order are fixed by the chunk bounds, lanes combine through a fixed DPP pattern, waves through LDS
// in wave order, chunks in chunk order.  The same inputs therefore give bitwise the same weights on every run.
//
// Segment offsets are 4-element aligned, so an fp32 chunk starts on a 16-byte boundary; the bf16 gradients of lp mode
// are read 8 per 16-byte load, from the 8-aligned index at or below the chunk's start.  A group of 4 (8) elements that
// is not entirely inside [lo, hi) -- the chunk's ragged end at `numel`, or the 4-element head of a bf16 chunk -- is
// read and written element by element under the bounds, so padding is never part of a norm and is never written.
//
// `state` (optional) is the clip state plx_gradnorm_finalize published for this step (train_kernels.hip): the gradient
// is multiplied by state[1] as a rounding step of its own, and state[3] != 0 (skipped step) leaves weights, moments
// and ratios alone: only the gradients are zeroed.
//
// hp layouts are the optimizers' own (train_kernels.hip): SGD [0] lr [1] momentum [2] weight_decay [3] nesterov
// [4] dampening [6] trust_coef; AdamW [0] lr [1] beta1 [2] beta2 [3] eps [4] weight_decay.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLX_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 16384;  // elements: 16 float4 (8 groups of 8 in lp mode) per lane
constexpr int kGridCap = 2048;

enum Mode { kLars = 0, kLamb = 1, kLambLp = 2 };

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf16_to_f(unsigned short h) { return __uint_as_float((uint32_t)h << 16); }

__device__ __forceinline__ unsigned short f_to_bf16(float f) {  // hardware RNE conversion (v_cvt_pk_bf16_f32)
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}

// ---------------------------------------------------------------- groups of VEC elements at an aligned index
// `full`: the group lies inside [lo, hi) and moves as 16-byte vectors; otherwise only the elements inside do.
template <int VEC>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, int64_t i, bool full, int64_t lo, int64_t hi,
                                         float (&x)[VEC]) {
  if (full) {
#pragma unroll
    for (int h = 0; h < VEC / 4; ++h) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p + i + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[4 * h + e] = t[e];
    }
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      x[k] = 0.f;
      if (i + k >= lo && i + k < hi) x[k] = p[i + k];
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_f32(float* __restrict__ p, int64_t i, bool full, int64_t lo, int64_t hi,
                                          const float (&x)[VEC]) {
  if (full) {
#pragma unroll
    for (int h = 0; h < VEC / 4; ++h)
      *reinterpret_cast<f32x4*>(p + i + 4 * h) = f32x4{x[4 * h], x[4 * h + 1], x[4 * h + 2], x[4 * h + 3]};
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (i + k >= lo && i + k < hi) p[i + k] = x[k];
  }
}

// The gradient: 4 fp32 or 8 bf16 per group, 16 bytes either way.
template <bool LP>
__device__ __forceinline__ void load_grad(const void* __restrict__ g, int64_t i, bool full, int64_t lo, int64_t hi,
                                          float (&x)[LP ? 8 : 4]) {
  if constexpr (LP) {
    const unsigned short* __restrict__ gb = static_cast<const unsigned short*>(g);
    if (full) {
      const u16x8 t = *reinterpret_cast<const u16x8*>(gb + i);
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = bf16_to_f(t[k]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        x[k] = 0.f;
        if (i + k >= lo && i + k < hi) x[k] = bf16_to_f(gb[i + k]);
      }
    }
  } else {
    load_f32<4>(static_cast<const float*>(g), i, full, lo, hi, x);
  }
}

template <bool LP>
__device__ __forceinline__ void zero_grad(void* __restrict__ g, int64_t i, bool full, int64_t lo, int64_t hi) {
  if constexpr (LP) {
    unsigned short* __restrict__ gb = static_cast<unsigned short*>(g);
    if (full) {
      *reinterpret_cast<u16x8*>(gb + i) = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (i + k >= lo && i + k < hi) gb[i + k] = 0;
    }
  } else {
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    store_f32<4>(static_cast<float*>(g), i, full, lo, hi, z);
  }
}

// ---------------------------------------------------------------- the per-element arithmetic, every rounding explicit
// (no contraction left to the compiler: the norm pass and the update pass must form bitwise the same u)
__device__ __forceinline__ float scale_grad(float g, float s) {
#pragma clang fp contract(off)
  return g * s;
}

struct AdamCoef {
  float lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2;
};

__device__ __forceinline__ AdamCoef adam_coef(const float* __restrict__ hp, const int* __restrict__ step_ptr) {
  AdamCoef c;
  c.lr = hp[0], c.b1 = hp[1], c.b2 = hp[2], c.eps = hp[3], c.wd = hp[4];
  const float t = (float)(*step_ptr + 1);
  c.inv_bc1 = 1.f / (1.f - __powf(c.b1, t));
  c.inv_sqrt_bc2 = rsqrtf(1.f - __powf(c.b2, t));
  return c;
}

__device__ __forceinline__ void adam_moments(float& m, float& v, float g, const AdamCoef& c) {
#pragma clang fp contract(off)
  m = fmaf(c.b1, m, (1.f - c.b1) * g);
  v = fmaf(c.b2, v, ((1.f - c.b2) * g) * g);
}

// u = m^ / (sqrt(v^) + eps) + wd w
__device__ __forceinline__ float lamb_u(float w, float m, float v, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float denom = fmaf(sqrtf(v), c.inv_sqrt_bc2, c.eps);
  return fmaf(c.wd, w, (m * c.inv_bc1) / denom);
}

// ---------------------------------------------------------------- block reduction of two sums
// Lanes combine by DPP inside the wave: two quad permutes, the half-row and row mirrors (every lane of a row of 16
// then holds the row's sum), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 -- lane 63 holds the
// wave's sum.  A masked-out row adds the 0 of `old`.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}

__device__ __forceinline__ float wave_sum_lane63(float v) {
  v = dpp_add<0xB1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4E, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x141, 0xf>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xf>(v);  // row_mirror
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31
  return v;
}

// out[0], out[1] = the block's sums of a and b, waves added in wave order.  Every thread of the block calls it.
__device__ __forceinline__ void block_sum2_store(float a, float b, float* __restrict__ out) {
  __shared__ float part[kWaves][2];
  a = wave_sum_lane63(a);
  b = wave_sum_lane63(b);
  if ((threadIdx.x & 63) == 63) {
    part[threadIdx.x >> 6][0] = a;
    part[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = part[0][0], tb = part[0][1];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) {
      ta += part[k][0];
      tb += part[k][1];
    }
    out[0] = ta;
    out[1] = tb;
  }
  __syncthreads();  // `part` is free again for the block's next chunk
}

// ---------------------------------------------------------------- pass 1: the two sums of squares of every chunk
template <int MODE>
__global__ __launch_bounds__(kBlock) void lw_norm_kernel(const float* __restrict__ w, const void* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const int64_t* __restrict__ chunk_lo,
                                                         const int64_t* __restrict__ chunk_hi, int n_chunks,
                                                         const float* __restrict__ hp,
                                                         const int* __restrict__ step_ptr,
                                                         const float* __restrict__ state,
                                                         float* __restrict__ partials) {
  constexpr bool LP = MODE == kLambLp;
  constexpr int VEC = LP ? 8 : 4;
  if (state != nullptr && state[3] != 0.f) return;  // skipped step: the moments must not advance
  const float scale = state != nullptr ? state[1] : 1.f;
  [[maybe_unused]] AdamCoef c;
  if constexpr (MODE != kLars) c = adam_coef(hp, step_ptr);
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t lo = chunk_lo[ch], hi = chunk_hi[ch];
    float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (lo & ~(int64_t)(VEC - 1)) + (int64_t)threadIdx.x * VEC; i < hi; i += (int64_t)kBlock * VEC) {
      const bool full = i >= lo && i + VEC <= hi;
      float wv[VEC], gv[VEC];
      load_f32<VEC>(w, i, full, lo, hi, wv);
      load_grad<LP>(g, i, full, lo, hi, gv);
      if constexpr (MODE == kLars) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float gk = scale_grad(gv[k], scale);
          sa[k & 3] = fmaf(wv[k], wv[k], sa[k & 3]);
          sb[k & 3] = fmaf(gk, gk, sb[k & 3]);
        }
      } else {
        float mv[VEC], vv[VEC];
        load_f32<VEC>(m, i, full, lo, hi, mv);
        load_f32<VEC>(v, i, full, lo, hi, vv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          adam_moments(mv[k], vv[k], scale_grad(gv[k], scale), c);
          // an element outside [lo, hi) was loaded as w = m = v = g = 0; its u would be 0 / eps, NaN at eps = 0
          const float u = (full || (i + k >= lo && i + k < hi)) ? lamb_u(wv[k], mv[k], vv[k], c) : 0.f;
          sa[k & 3] = fmaf(wv[k], wv[k], sa[k & 3]);
          sb[k & 3] = fmaf(u, u, sb[k & 3]);
        }
        store_f32<VEC>(m, i, full, lo, hi, mv);
        store_f32<VEC>(v, i, full, lo, hi, vv);
      }
    }
    block_sum2_store((sa[0] + sa[1]) + (sa[2] + sa[3]), (sb[0] + sb[1]) + (sb[2] + sb[3]), partials + 2 * (int64_t)ch);
  }
}

// ---------------------------------------------------------------- pass 2: one wave per segment -> its trust ratio
// LARS  r = trust_coef |w| / (|g| + wd |w| + 1e-8)     LAMB  r = |w| / |u|     r = 1 unless both norms are positive
template <bool LAMB>
__global__ __launch_bounds__(64) void lw_ratio_kernel(const float* __restrict__ partials,
                                                      const int* __restrict__ seg_first,
                                                      const int* __restrict__ seg_count,
                                                      const float* __restrict__ hp, const float* __restrict__ state,
                                                      float* __restrict__ ratio) {
  if (state != nullptr && state[3] != 0.f) return;
  const int s = blockIdx.x;
  const int first = seg_first[s], count = seg_count[s];
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < count; k += 64) {
    a += (double)partials[2 * (int64_t)(first + k)];
    b += (double)partials[2 * (int64_t)(first + k) + 1];
  }
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(a), xn = (float)sqrt(b);
    float r = 1.f;
    if (wn > 0.f && xn > 0.f) {
      if constexpr (LAMB)
        r = wn / xn;
      else
        r = hp[6] * wn / (xn + hp[2] * wn + 1e-8f);
    }
    ratio[s] = r;
  }
}

// ---------------------------------------------------------------- pass 3: the update of every chunk
template <int MODE>
__global__ __launch_bounds__(kBlock) void lw_update_kernel(float* __restrict__ w, void* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           unsigned short* __restrict__ wlp,
                                                           const int64_t* __restrict__ chunk_lo,
                                                           const int64_t* __restrict__ chunk_hi,
                                                           const int* __restrict__ chunk_seg, int n_chunks,
                                                           const float* __restrict__ ratio,
                                                           const float* __restrict__ hp,
                                                           const int* __restrict__ step_ptr,
                                                           const float* __restrict__ state) {
  constexpr bool LP = MODE == kLambLp;
  constexpr int VEC = LP ? 8 : 4;
  const bool skip = state != nullptr && state[3] != 0.f;
  const float scale = state != nullptr ? state[1] : 1.f;
  // LARS: the SGD hyper-parameters; `first`: the step after (re)initialisation, momentum := d
  [[maybe_unused]] const float lr = hp[0], mom = hp[1], wd = hp[2], damp = hp[4];
  [[maybe_unused]] const bool nesterov = hp[3] != 0.f;
  [[maybe_unused]] const bool first = *step_ptr == 0;
  [[maybe_unused]] AdamCoef c;
  if constexpr (MODE != kLars) c = adam_coef(hp, step_ptr);
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t lo = chunk_lo[ch], hi = chunk_hi[ch];
    const float r = skip ? 1.f : ratio[chunk_seg[ch]];
    for (int64_t i = (lo & ~(int64_t)(VEC - 1)) + (int64_t)threadIdx.x * VEC; i < hi; i += (int64_t)kBlock * VEC) {
      const bool full = i >= lo && i + VEC <= hi;
      if (skip) {
        zero_grad<LP>(g, i, full, lo, hi);
        continue;
      }
      float wv[VEC], mv[VEC];
      load_f32<VEC>(w, i, full, lo, hi, wv);
      load_f32<VEC>(m, i, full, lo, hi, mv);
      if constexpr (MODE == kLars) {
        float gv[VEC];
        load_grad<LP>(g, i, full, lo, hi, gv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float d = r * fmaf(wd, wv[k], scale_grad(gv[k], scale));
          mv[k] = first ? d : mom * mv[k] + (1.f - damp) * d;
          wv[k] -= lr * (nesterov ? d + mom * mv[k] : mv[k]);
        }
        store_f32<VEC>(m, i, full, lo, hi, mv);
      } else {
        float vv[VEC];
        load_f32<VEC>(v, i, full, lo, hi, vv);
        const float step_size = c.lr * r;
#pragma unroll
        for (int k = 0; k < VEC; ++k) wv[k] = fmaf(-step_size, lamb_u(wv[k], mv[k], vv[k], c), wv[k]);
      }
      store_f32<VEC>(w, i, full, lo, hi, wv);
      if constexpr (LP) {
        if (full) {
          u16x8 lp;
#pragma unroll
          for (int k = 0; k < 8; ++k) lp[k] = f_to_bf16(wv[k]);
          *reinterpret_cast<u16x8*>(wlp + i) = lp;
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (i + k >= lo && i + k < hi) wlp[i + k] = f_to_bf16(wv[k]);
        }
      }
      zero_grad<LP>(g, i, full, lo, hi);
    }
  }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

inline int grid_for_chunks(int n_chunks) { return n_chunks < kGridCap ? n_chunks : kGridCap; }

}  // namespace

// Elements per chunk: the host builds the chunk table with it.
PLX_API int plx_lw_chunk() { return kChunk; }

// mode 0 LARS (g fp32; m, v, step unused), 1 LAMB (g fp32), 2 LAMB lp (g bf16).  Chunk c covers flat elements
// [chunk_lo[c], chunk_hi[c]) of one segment, chunk_lo 4-aligned, at most plx_lw_chunk() elements; every buffer is
// indexed by the flat element and 16-byte aligned.  partials holds 2 * n_chunks floats.
PLX_API int plx_lw_norms(int mode, const float* w, const void* g, float* m, float* v, const int64_t* chunk_lo,
                         const int64_t* chunk_hi, int n_chunks, const float* hp, const int* step,
                         const float* state, float* partials, hipStream_t stream) {
  if (n_chunks == 0) return 0;
  if (n_chunks < 0 || !w || !g || !chunk_lo || !chunk_hi || !hp || !partials) return 1;
  if (!aligned16(w) || !aligned16(g) || !aligned16(m) || !aligned16(v)) return 1;
  if (mode != kLars && (!m || !v || !step)) return 1;
  const dim3 grid(grid_for_chunks(n_chunks)), block(kBlock);
  if (mode == kLars)
    hipLaunchKernelGGL(lw_norm_kernel<kLars>, grid, block, 0, stream, w, g, m, v, chunk_lo, chunk_hi, n_chunks, hp,
                       step, state, partials);
  else if (mode == kLamb)
    hipLaunchKernelGGL(lw_norm_kernel<kLamb>, grid, block, 0, stream, w, g, m, v, chunk_lo, chunk_hi, n_chunks, hp,
                       step, state, partials);
  else if (mode == kLambLp)
    hipLaunchKernelGGL(lw_norm_kernel<kLambLp>, grid, block, 0, stream, w, g, m, v, chunk_lo, chunk_hi, n_chunks, hp,
                       step, state, partials);
  else
    return 1;
  return (int)hipGetLastError();
}

// ratio[s] from the partials of chunks [seg_first[s], seg_first[s] + seg_count[s]); lamb: 0 LARS, 1 LAMB.
PLX_API int plx_lw_ratios(int lamb, const float* partials, const int* seg_first, const int* seg_count, int n_seg,
                          const float* hp, const float* state, float* ratio, hipStream_t stream) {
  if (n_seg == 0) return 0;
  if (n_seg < 0 || !partials || !seg_first || !seg_count || !hp || !ratio) return 1;
  if (lamb)
    hipLaunchKernelGGL(lw_ratio_kernel<true>, dim3(n_seg), dim3(64), 0, stream, partials, seg_first, seg_count, hp,
                       state, ratio);
  else
    hipLaunchKernelGGL(lw_ratio_kernel<false>, dim3(n_seg), dim3(64), 0, stream, partials, seg_first, seg_count, hp,
                       state, ratio);
  return (int)hipGetLastError();
}

// The update of every chunk with its segment's ratio (chunk_seg[c]).  LARS: m is the momentum buffer, step the
// first-step counter, v and wlp unused.  LAMB lp: wlp is the bf16 model copy, rewritten from the new master weights.
PLX_API int plx_lw_update(int mode, float* w, void* g, float* m, float* v, void* wlp, const int64_t* chunk_lo,
                          const int64_t* chunk_hi, const int* chunk_seg, int n_chunks, const float* ratio,
                          const float* hp, const int* step, const float* state, hipStream_t stream) {
  if (n_chunks == 0) return 0;
  if (n_chunks < 0 || !w || !g || !m || !chunk_lo || !chunk_hi || !chunk_seg || !ratio || !hp || !step) return 1;
  if (!aligned16(w) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(wlp)) return 1;
  if (mode != kLars && !v) return 1;
  if (mode == kLambLp && !wlp) return 1;
  const dim3 grid(grid_for_chunks(n_chunks)), block(kBlock);
  unsigned short* lp = static_cast<unsigned short*>(wlp);
  if (mode == kLars)
    hipLaunchKernelGGL(lw_update_kernel<kLars>, grid, block, 0, stream, w, g, m, v, lp, chunk_lo, chunk_hi, chunk_seg,
                       n_chunks, ratio, hp, step, state);
  else if (mode == kLamb)
    hipLaunchKernelGGL(lw_update_kernel<kLamb>, grid, block, 0, stream, w, g, m, v, lp, chunk_lo, chunk_hi, chunk_seg,
                       n_chunks, ratio, hp, step, state);
  else if (mode == kLambLp)
    hipLaunchKernelGGL(lw_update_kernel<kLambLp>, grid, block, 0, stream, w, g, m, v, lp, chunk_lo, chunk_hi,
                       chunk_seg, n_chunks, ratio, hp, step, state);
  else
    return 1;
  return (int)hipGetLastError();
}
