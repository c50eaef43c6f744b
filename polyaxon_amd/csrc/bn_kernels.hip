// Fused BatchNorm(+residual add)(+ReLU) for NHWC bf16 activations on MI355X (gfx950).
//
// A ResNet-50 training step runs 53 BatchNorms, 49 of them followed by ReLU and 16 by a residual add
// first.  Unfused, that is stats + normalise + add + relu in the forward and relu-backward + BN-backward
// (+ the add's gradient copy) in the backward: 7-9 full passes over each activation, all HBM-bound.
// These kernels do it in 2 passes forward (stats, apply) and 2 backward (reduce, dx), 16-byte vectors
// (8 x bf16) per lane, fp32 math, fp32 per-channel partials.
//
// Layout: x viewed as [M, C] row-major, M = N*H*W (channels_last), C % 8 == 0 and C/8 a power of two.
// Thread t of a 256-thread block owns channel group cg = t % Gb (8 channels, Gb = min(C/8, 256)) and row
// lane t / Gb, so its per-channel state (shift, scale, bias, mean, invstd) stays in registers while it
// walks rows; one wave reads 64 x 16 B = 1 KiB contiguous per instruction.
//
//   bn_stats_kernel                per-block shifted sum / sum-of-squares partials [2][nblk][C]
//   bn_fwd_reduce_finalize_kernel  level-2 reduce, then mean, invstd, fused scale/bias, running stats (unbiased var)
//   bn_apply_kernel                y = act(x*scale + bias [+ res]), and the 1-bit ReLU mask
//   bn_bwd_reduce_kernel           partial sums of dz and dz*xhat   (dz = dy * [y > 0] when act)
//   bn_bwd_reduce_finalize_kernel  level-2 reduce, then dgamma, dbeta and the dx coefficients  dx = A*dz + B*x + D
//   bn_bwd_dx_kernel               dx (and d_residual = dz where asked for) in one pass, optionally with the reduction
//                                  partials of the BatchNorm that produced the residual (ResBn: a downsampling
//                                  branch's BN skips its reduce)
//   (without a counter array a reduce + finalize is bn_partial_reduce_kernel + bn_{fwd,bwd}_finalize_kernel)
// Entry points: plx_bn_forward / plx_bn_backward (one argument struct each), plx_bn_apply, plx_bn_apply_res_relu, the
// stem's plx_stem_bn_pool_forward / _backward (stem_*_kernel), and the size queries (plx_bn_workspace, ...).
#include <hip/hip_runtime.h>

#include "handoff.h"
#include <stdint.h>
#include <type_traits>

#define PLX_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kBlock = 256;

struct alignas(16) bf16x8 {
  uint16_t v[8];
};

__device__ __forceinline__ float bf2f(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }

__device__ __forceinline__ uint16_t f2bf(float f) {  // round-to-nearest-even, NaN stays NaN
  // a plain cast: hipcc emits v_cvt_pk_bf16_f32 (MI355X_MICROARCH.md, correctness table) -- one instruction where the
  // integer form was ~6, which showed in the VALU-heavy passes (fused stem forward 342 -> 284 us)
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}

__device__ __forceinline__ void load8(const bf16x8* p, float* f) {
  const bf16x8 v = *p;
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = bf2f(v.v[k]);
}

__device__ __forceinline__ void store8(bf16x8* p, const float* f) {
  bf16x8 v;
#pragma unroll
  for (int k = 0; k < 8; ++k) v.v[k] = f2bf(f[k]);
  *p = v;
}

// ------------------------------------------------------------------------------- forward stats
__global__ __launch_bounds__(kBlock) void bn_stats_kernel(const bf16x8* __restrict__ x, int64_t M, int G, int Gb,
                                                          int64_t rows_per_block, float* __restrict__ psum,
                                                          float* __restrict__ psq) {
  __shared__ float s_sum[kBlock * 8];
  __shared__ float s_sq[kBlock * 8];
  const int tid = threadIdx.x;
  const int cg_local = tid % Gb, rlane = tid / Gb, R = kBlock / Gb;
  const int cg = blockIdx.y * Gb + cg_local;
  const int C = G * 8;
  float shift[8], s[8], q[8];
  load8(x + cg, shift);  // row 0 as the shift: var = E[(x-k)^2] - E[x-k]^2 stays well conditioned
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = q[k] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > M) r1 = M;
#pragma unroll 4
  for (int64_t r = r0 + rlane; r < r1; r += R) {
    float v[8];
    load8(x + r * G + cg, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = v[k] - shift[k];
      s[k] += d;
      q[k] = fmaf(d, d, q[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    s_sum[tid * 8 + k] = s[k];
    s_sq[tid * 8 + k] = q[k];
  }
  __syncthreads();
  if (rlane == 0) {
    for (int j = 1; j < R; ++j) {
      const int o = (j * Gb + cg_local) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s[k] += s_sum[o + k];
        q[k] += s_sq[o + k];
      }
    }
    float* ps = psum + (int64_t)blockIdx.x * C + cg * 8;
    float* pq = psq + (int64_t)blockIdx.x * C + cg * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ps[k] = s[k];
      pq[k] = q[k];
    }
  }
}

// Level-2 reduction of the per-block partials: [2][nblk][C] -> [2][S][C], S = ceil(nblk / 64).
// Block = 64 channels x 4 row lanes (one wave reads 64 consecutive channels = 256 B per row), grid
// (ceil(C/64), S, 2): parallel over channels AND partial rows, so neither a large C (layer4) nor a
// large nblk (stem) leaves the reduction on a handful of CUs.
constexpr int kRowsPerSplit = 64;

// Per thread: the U = kRowsPerSplit / G rows lane, lane + G, ... of split s, all loads issued at once, summed in
// row order; the G group sums are then combined in group order.  bn_partial_reduce_kernel<NT> and the one-launch
// reduce_l2_last<NT> share this arithmetic, so both paths give bit-identical level-2 rows.
template <int NT>
__device__ __forceinline__ float l1_rows(const float* __restrict__ src, int b0, int b1, int C, int c, int lane) {
  constexpr int G = NT / 64, U = kRowsPerSplit / G;
  float x[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int b = b0 + lane + u * G;
    x[u] = b < b1 ? src[(int64_t)b * C + c] : 0.f;
  }
  float a = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) a += x[u];
  return a;
}

template <int NT>
__global__ __launch_bounds__(NT) void bn_partial_reduce_kernel(const float* __restrict__ part, int nblk, int C,
                                                               float* __restrict__ out, int S) {
  constexpr int G = NT / 64;
  __shared__ float sh[NT];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int lane = threadIdx.x >> 6;
  const int s = blockIdx.y, which = blockIdx.z;
  const int b0 = s * kRowsPerSplit;
  const int b1 = b0 + kRowsPerSplit < nblk ? b0 + kRowsPerSplit : nblk;
  sh[threadIdx.x] = c < C ? l1_rows<NT>(part + (int64_t)which * nblk * C, b0, b1, C, c, lane) : 0.f;
  __syncthreads();
  if (lane == 0 && c < C) {
    float r = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) r += sh[threadIdx.x + 64 * g];
    out[((int64_t)which * S + s) * C + c] = r;
  }
}

// Level-2 -> per-channel totals for the finalize kernels: block = 64 channels x 4 split lanes-groups, each group
// sums every 4th of the S partial rows (independent loads, fp64 accumulation), then the 4 group sums are combined
// through LDS in a fixed order (deterministic).  One thread per channel walking all S rows serially was 19 us per
// backward BatchNorm on the 56x56 layers (S ~ 100 dependent-latency iterations on a single 256-thread block).
// ATOMIC: the rows were published inside this launch by other workgroups (agent-scope atomic stores): read them with
// agent-scope atomic loads (coherent across the XCDs' L2s without an acquire fence / L2 invalidate)
template <int NT = 256, bool ATOMIC = false>
__device__ __forceinline__ bool fin_sum2(const float* __restrict__ pa, const float* __restrict__ pb, int nblk, int C,
                                         double& A, double& B) {
  constexpr int G = NT / 64;  // split lane-groups
  __shared__ double sh[2][G][64];
  const int lc = threadIdx.x & 63, sp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lc;
  double a0 = 0.0, b0 = 0.0;
  if (c < C) {
    // 8 rows (16 predicated loads) in flight per trip: this runs in the last-arriving block, on the critical path of
    // every BatchNorm; with 16 groups (1024 threads) S <= 128 level-2 rows is ONE dependent L2 round trip
    for (int b = sp; b < nblk; b += 8 * G) {
      float x[8], y[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = b + u * G;
        if (ATOMIC) {
          x[u] = r < nblk ? __hip_atomic_load(pa + (int64_t)r * C + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
          y[u] = r < nblk ? __hip_atomic_load(pb + (int64_t)r * C + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        } else {
          x[u] = r < nblk ? pa[(int64_t)r * C + c] : 0.f;
          y[u] = r < nblk ? pb[(int64_t)r * C + c] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { a0 += x[u]; b0 += y[u]; }
    }
  }
  sh[0][sp][lc] = a0;
  sh[1][sp][lc] = b0;
  __syncthreads();
  if (sp != 0 || c >= C) return false;
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) { sa += sh[0][g][lc]; sb += sh[1][g][lc]; }  // fixed order: deterministic
  A = sa;
  B = sb;
  return true;
}

struct FwdFin {
  const uint16_t* x_row0;  // shift of the stats pass (nullptr: producer-fused, unshifted sums)
  int C;
  int64_t M;
  const float* gamma;
  const float* beta;
  float eps, momentum;
  float* running_mean;
  float* running_var;
  float* save_mean;
  float* save_invstd;
  float* scale;
  float* bias;
};

struct BwdFin {
  int C;
  int64_t M;
  const float* gamma;
  const float* mean;
  const float* invstd;
  float* dgamma;
  float* dbeta;
  float* coef;
  int accumulate;
};

// The per-channel values a finalize reads besides the sums.  None depends on the sums, so the one-launch kernels load
// them BEFORE the partial rows: behind the sums each was one more dependent round trip on the critical path of every
// BatchNorm, dbeta / dgamma's two behind a branch on `accumulate`.  Every load is unconditional: dgamma / dbeta are
// read whatever `accumulate` says and the value is dropped when it is not wanted.
struct FwdPar {
  float gamma, beta, rmean, rvar, x0;
};

struct BwdPar {
  float gamma, mean, invstd, dgamma, dbeta;
};

// A raw buffer descriptor over `bytes` bytes at p (wave-uniform inputs only): a load through it at an offset >= bytes
// reads nothing and returns 0.  That is how these kernels drop a value without a select on it: hipcc turns
// `ok ? p[i] : 0.f` into a branch around the load with an `s_waitcnt vmcnt(0)` behind it, one dependent round trip
// per row (cdna_hip_programming.md, buffer addressing)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// p[c] for the lanes that are `on`, +0 (and no access) for the others and for a null p: nothing is predicated, so
// every wave issues these loads and moves on
__device__ __forceinline__ float par_load(const float* p, int C, int c, bool on) {
  const int bytes = p != nullptr ? C * (int)sizeof(float) : 0;
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(p, bytes), on ? c * (int)sizeof(float) : bytes, 0, 0));
}

// on: this thread finalizes channel c if any thread of its block does
__device__ __forceinline__ FwdPar fwd_params(const FwdFin& f, int c, bool on) {
  FwdPar p;
  p.gamma = par_load(f.gamma, f.C, c, on);
  p.beta = par_load(f.beta, f.C, c, on);
  p.rmean = par_load(f.running_mean, f.C, c, on);
  p.rvar = par_load(f.running_mean != nullptr ? f.running_var : nullptr, f.C, c, on);
  const int xbytes = f.x_row0 != nullptr ? 2 * f.C : 0;  // null x_row0: 0 = +0.f
  p.x0 = bf2f((uint16_t)__builtin_amdgcn_raw_buffer_load_b16(buf_rsrc(f.x_row0, xbytes), on ? 2 * c : xbytes, 0, 0));
  return p;
}

__device__ __forceinline__ BwdPar bwd_params(const BwdFin& f, int c, bool on) {
  BwdPar p;
  p.gamma = par_load(f.gamma, f.C, c, on);
  p.mean = par_load(f.mean, f.C, c, on);
  p.invstd = par_load(f.invstd, f.C, c, on);
  p.dgamma = par_load(f.dgamma, f.C, c, on);
  p.dbeta = par_load(f.dbeta, f.C, c, on);
  return p;
}

// Everything after the sums: S, Q are channel c's fp64 totals of the shifted sum and sum of squares
__device__ __forceinline__ void fwd_finish(const FwdFin& f, int c, double S, double Q, const FwdPar& p) {
  const double m = S / (double)f.M;
  double var = Q / (double)f.M - m * m;
  if (var < 0.0) var = 0.0;
  const float mean = p.x0 + (float)m;
  const float invstd = rsqrtf((float)var + f.eps);
  const float g = p.gamma;
  f.save_mean[c] = mean;
  f.save_invstd[c] = invstd;
  f.scale[c] = g * invstd;
  f.bias[c] = p.beta - mean * g * invstd;
  if (f.running_mean != nullptr) {
    const float unbiased = f.M > 1 ? (float)(var * (double)f.M / (double)(f.M - 1)) : (float)var;
    f.running_mean[c] = (1.f - f.momentum) * p.rmean + f.momentum * mean;
    f.running_var[c] = (1.f - f.momentum) * p.rvar + f.momentum * unbiased;
  }
}

// A, B: channel c's fp64 totals of dz and dz * xhat
__device__ __forceinline__ void bwd_finish(const BwdFin& f, int c, double A, double B, const BwdPar& p) {
  const int C = f.C;
  const float db = (float)A, dg = (float)B;
  // accumulate: dgamma / dbeta are the parameters' own (flat) gradient slots, summed into like autograd would
  f.dbeta[c] = f.accumulate ? p.dbeta + db : db;
  f.dgamma[c] = f.accumulate ? p.dgamma + dg : dg;
  const float is = p.invstd, k1 = p.gamma * is;
  const float k2 = db / (float)f.M, k3 = dg / (float)f.M;
  // dx = k1 * (dz - k2 - xhat*k3),  xhat = (x - mean) * is   =>  dx = A*dz + B*x + D
  f.coef[c] = k1;                                    // A
  f.coef[C + c] = -k1 * k3 * is;                     // B
  f.coef[2 * C + c] = -k1 * k2 + k1 * k3 * is * p.mean;  // D
}

template <int NT, bool ATOMIC = false>
__device__ __forceinline__ void fwd_finalize(const float* psum, const float* psq, int nblk, const FwdFin& f,
                                             const FwdPar& p) {
  double S, Q;  // level-2 partials per channel, summed in fp64
  if (!fin_sum2<NT, ATOMIC>(psum, psq, nblk, f.C, S, Q)) return;
  fwd_finish(f, blockIdx.x * 64 + (threadIdx.x & 63), S, Q, p);
}

template <int NT, bool ATOMIC = false>
__device__ __forceinline__ void bwd_finalize(const float* pdz, const float* pdzx, int nblk, const BwdFin& f,
                                             const BwdPar& p) {
  double A, B;
  if (!fin_sum2<NT, ATOMIC>(pdz, pdzx, nblk, f.C, A, B)) return;
  bwd_finish(f, blockIdx.x * 64 + (threadIdx.x & 63), A, B, p);
}

// Level-1 -> level-2 reduce and the finalize in ONE launch: grid (ceil(C/64), S), every block reduces its 64 partial
// rows of both sums for 64 channels (same order as bn_partial_reduce_kernel), publishes them, and takes a ticket on
// its channel group's counter; the block drawing S-1 runs the finalize over the S level-2 rows.  The hand-off is
// the split-K last-arriver recipe (cdna_hip_programming.md §5, in-launch split-K reduction): plain stores, every
// wave drained, agent-scope release by one lane before a relaxed agent-scope ticket add, agent-scope acquire by the
// last arriver before the workgroup reads.  Counters start at zero (allocated zeroed) and the last arriver resets
// its own; launches that share a counter array are stream-ordered.  Saves a launch boundary and the separate
// finalize pass's own ramp per BatchNorm direction (106 per ResNet-50 step).
// l1_rows<NT> with every load unconditional: a buffer over the split's rows b0 .. b1 - 1, so a row past b1 lies past
// its end and reads as +0 (a channel past C is sent there too).  Same values, same order, one round trip where the
// predicated loads of l1_rows compile to three
template <int NT>
__device__ __forceinline__ float l1_rows_buf(const float* __restrict__ src, int b0, int b1, int C, int c, int lane) {
  constexpr int G = NT / 64, U = kRowsPerSplit / G;
  const int bytes = (b1 - b0) * C * (int)sizeof(float);
  const __amdgpu_buffer_rsrc_t r = buf_rsrc(src + (int64_t)b0 * C, bytes);
  float x[U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    x[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
        r, c < C ? ((lane + u * G) * C + c) * (int)sizeof(float) : bytes, 0, 0));
  float a = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) a += x[u];
  return a;
}

template <int NT>
__device__ __forceinline__ bool reduce_l2_last(const float* __restrict__ part, int nblk, int C, float* l2, int S,
                                               unsigned* cnt) {
  constexpr int G = NT / 64;
  __shared__ float sh[2][NT];
  __shared__ int s_last;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int lane = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int b0 = s * kRowsPerSplit;
  int b1 = b0 + kRowsPerSplit;
  if (b1 > nblk) b1 = nblk;
  const float a0 = l1_rows_buf<NT>(part, b0, b1, C, c, lane);
  const float a1 = l1_rows_buf<NT>(part + (int64_t)nblk * C, b0, b1, C, c, lane);
  sh[0][threadIdx.x] = a0;
  sh[1][threadIdx.x] = a1;
  __syncthreads();
  if (lane == 0 && c < C) {
    const int t = threadIdx.x;
    float r0 = 0.f, r1 = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) { r0 += sh[0][t + 64 * g]; r1 += sh[1][t + 64 * g]; }
    // agent-scope atomic stores: coherent across the XCDs' L2s, so no release fence (an L2 write-back per
    // workgroup on gfx950) and, on the reading side, no acquire fence (an L2 invalidate): atomic loads instead
    __hip_atomic_store(l2 + (int64_t)s * C + c, r0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(l2 + ((int64_t)S + s) * C + c, r1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains
  __syncthreads();
  if (threadIdx.x == 0) {
    plx_handoff_release();  // no-op unless built with PLX_HANDOFF_FENCES (csrc/handoff.h: the hardware assumption)
    const unsigned old = __hip_atomic_fetch_add(cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == (unsigned)(S - 1);
    if (last) plx_handoff_acquire();
    if (last) __hip_atomic_store(cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}

// 1024 threads: 16 row groups make both the level-1 rows (4 per thread) and the S level-2 rows (<= 8 per thread
// up to S = 128) a single L2 round trip each; with 256 threads they were 2 and up to 4 dependent trips
constexpr int kFinNT = 1024;
// (round 6 removed the 256-thread finalize variant: -0.5 %, profiles/r5_knob_recheck_ab.jsonl)
template <int NT>
__global__ __launch_bounds__(NT) void bn_fwd_reduce_finalize_kernel(const float* __restrict__ part, int nblk, float* l2,
                                                                    int S, unsigned* cnt, FwdFin f) {
  // the finalizing threads of the last arriver are the first wave's; every block loads for them, which block is last
  // is not known yet
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const FwdPar p = fwd_params(f, c, threadIdx.x < 64 && c < f.C);
  if (!reduce_l2_last<NT>(part, nblk, f.C, l2, S, cnt)) return;
  fwd_finalize<NT, true>(l2, l2 + (int64_t)S * f.C, S, f, p);
}

template <int NT>
__global__ __launch_bounds__(NT) void bn_bwd_reduce_finalize_kernel(const float* __restrict__ part, int nblk, float* l2,
                                                                    int S, unsigned* cnt, BwdFin f) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const BwdPar p = bwd_params(f, c, threadIdx.x < 64 && c < f.C);
  if (!reduce_l2_last<NT>(part, nblk, f.C, l2, S, cnt)) return;
  bwd_finalize<NT, true>(l2, l2 + (int64_t)S * f.C, S, f, p);
}

// ---- reduce + finalize in ONE workgroup per CW channels, for the BatchNorms with few partial rows (nblk <= kFinSingleMax:
// the 14x14 and 7x7 stages of ResNet-50, 28 of its 53 BatchNorms).  There the ticket kernels above join only 2-7
// workgroups, yet pay for it with the level-2 stores, their drain, the ticket's atomic and the re-read of the rows:
// four dependent memory round trips that move almost no data.  Here every thread issues all of its level-1 loads of
// both sums (and wave 0 the per-channel parameters) before its first wait, the rest happens in LDS, and nothing but
// the outputs is written: no counters, no level-2 rows, no atomics.
//
// The summation tree is the ticket path's, so every output is bit-identical to it:
//   per split s of 64 rows, lane group g = 0..15 sums rows g, g + 16, g + 32, g + 48 in that order (l1_rows<kFinNT>),
//   the 16 group sums are added in group order (fp32): the level-2 value r_s;
//   fin_sum2<kFinNT> then adds r_0 .. r_{S-1} in order in fp64 (S <= 16: one row per lane group, groups in order).
// Thread t = j * CW + lc serves channel lc of the workgroup, lane group g = j % 16 and the splits sub, sub + NSUB, ...
// (sub = j / 16, NSUB = 64 / CW): a narrower workgroup spreads a BatchNorm over more CUs (C = 256 at CW = 64 is four
// workgroups, each pulling 200 KB through one CU's L2 port) and leaves each thread fewer rows, while a wave still
// reads 64 / CW whole rows of CW contiguous floats per instruction.
constexpr int kFinSingleSplits = 8;                               // splits of 64 rows one workgroup holds in flight
constexpr int kFinSingleMax = kFinSingleSplits * kRowsPerSplit;   // = 512 rows: 32 rows x 2 sums per thread at CW = 64

// SM: the splits the workgroup covers (>= S).  A row past nblk or a channel past C is read past the end of the buffer
// descriptor and comes back as +0 (buf_rsrc): every load is unconditional.
// load_params: the caller's parameter loads, issued behind the row loads (ahead of them the row offsets' 64-bit
// multiply-adds picked a parameter's register as their don't-care high half, and waited for it)
template <int CW, int SM, typename F>
__device__ __forceinline__ bool single_sum2(const float* __restrict__ part, int nblk, int C, double& A, double& B,
                                            F&& load_params) {
  constexpr int NT = kFinNT;
  constexpr int NSUB = 64 / CW;      // split lanes: thread groups that share (channel, lane group), each SM / NSUB splits
  constexpr int KS = SM / NSUB;      // splits per thread
  constexpr int RS = CW == 64 && SM > 4 ? 4 : SM;  // splits per LDS round: sh stays at 32 KB
  static_assert(NT / CW == 16 * NSUB && SM % NSUB == 0 && SM % RS == 0 && 2 * RS * CW <= NT && SM <= 16, "mapping");
  __shared__ float sh[2][RS][16][CW];
  __shared__ float rs[2][SM][CW];
  const int t = threadIdx.x;
  const int lc = t % CW, j = t / CW, g = j & 15, sub = j >> 4;
  const int c = blockIdx.x * CW + lc;
  const int bytes = 2 * nblk * C * (int)sizeof(float);  // < 2^31: fin_path
  const __amdgpu_buffer_rsrc_t src = buf_rsrc(part, bytes);
  float x[2][KS][4];
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int k = 0; k < KS; ++k)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = (sub + NSUB * k) * kRowsPerSplit + g + 16 * u;
        const int off = ((w * nblk + b) * C + c) * (int)sizeof(float);
        x[w][k][u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(src, b < nblk && c < C ? off : bytes, 0, 0));
      }
  load_params();
  // all of them are issued before anything waits: left alone the scheduler pulls the first round's LDS writes, and the
  // waits they need, in between the loads (two to three round trips instead of one)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r0 = 0; r0 < SM; r0 += RS) {
    if (r0 != 0) __syncthreads();  // the previous round's sh has been read
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
      for (int k = 0; k < KS; ++k) {
        float a = 0.f;  // l1_rows: rows in order
#pragma unroll
        for (int u = 0; u < 4; ++u) a += x[w][k][u];
        const int s = sub + NSUB * k;  // CW = 64: sub = 0, so the round test folds away
        if (s >= r0 && s < r0 + RS) sh[w][s - r0][g][lc] = a;
      }
    __syncthreads();
    if (t < 2 * RS * CW) {  // one (sum, split, channel) per thread: the 16 group sums in group order
      const int w = t / (RS * CW), sl = t / CW % RS;
      float r = 0.f;
#pragma unroll
      for (int gg = 0; gg < 16; ++gg) r += sh[w][sl][gg][lc];
      rs[w][r0 + sl][lc] = r;
    }
  }
  __syncthreads();
  if (t >= CW || c >= C) return false;
  // fin_sum2 over S <= 16 level-2 rows: r_0 .. r_{S-1} in order; the splits past S are +0 and change nothing
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int s = 0; s < SM; ++s) { sa += (double)rs[0][s][t]; sb += (double)rs[1][s][t]; }
  A = sa;
  B = sb;
  return true;
}

template <int CW, int SM>
__global__ __launch_bounds__(kFinNT) void bn_fwd_finalize_single_kernel(const float* __restrict__ part, int nblk,
                                                                        FwdFin f) {
  const int c = blockIdx.x * CW + threadIdx.x % CW;
  FwdPar p;
  double S, Q;
  if (!single_sum2<CW, SM>(part, nblk, f.C, S, Q, [&] { p = fwd_params(f, c, threadIdx.x < CW && c < f.C); })) return;
  fwd_finish(f, c, S, Q, p);
}

template <int CW, int SM>
__global__ __launch_bounds__(kFinNT) void bn_bwd_finalize_single_kernel(const float* __restrict__ part, int nblk,
                                                                        BwdFin f) {
  const int c = blockIdx.x * CW + threadIdx.x % CW;
  BwdPar p;
  double A, B;
  if (!single_sum2<CW, SM>(part, nblk, f.C, A, B, [&] { p = bwd_params(f, c, threadIdx.x < CW && c < f.C); })) return;
  bwd_finish(f, c, A, B, p);
}

template <int NT>
__global__ __launch_bounds__(NT) void bn_fwd_finalize_kernel(const float* __restrict__ psum, const float* __restrict__ psq, int nblk,
                                       const uint16_t* __restrict__ x_row0, int C, int64_t M,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                       float momentum, float* __restrict__ running_mean,
                                       float* __restrict__ running_var, float* __restrict__ save_mean,
                                       float* __restrict__ save_invstd, float* __restrict__ scale,
                                       float* __restrict__ bias) {
  double S, Q;  // level-2 partials per channel, summed in fp64
  if (!fin_sum2<NT>(psum, psq, nblk, C, S, Q)) return;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const double m = S / (double)M;
  double var = Q / (double)M - m * m;
  if (var < 0.0) var = 0.0;
  const float mean = (x_row0 != nullptr ? bf2f(x_row0[c]) : 0.f) + (float)m;  // no shift: producer-fused stats
  const float invstd = rsqrtf((float)var + eps);
  const float g = gamma[c];
  save_mean[c] = mean;
  save_invstd[c] = invstd;
  scale[c] = g * invstd;
  bias[c] = beta[c] - mean * g * invstd;
  if (running_mean != nullptr) {
    const float unbiased = M > 1 ? (float)(var * (double)M / (double)(M - 1)) : (float)var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// ------------------------------------------------------------------------------- forward apply
// RES / RELU are compile-time: with a runtime residual test hipcc waited for x's load before issuing the residual's
// (one extra HBM round trip per trip), and a per-element `rsb ? rsb[c] : 1` in the prologue became eight
// load-then-wait branches (cdna_hip_programming.md §5 item 4(c)) -- ~20 us of latency per block that dominated the
// 14x14 / 7x7 layers (35 us for a 53 MB apply, profiles/r2_resnet50_roofline.md).
template <bool RES, bool RELU>
__global__ __launch_bounds__(kBlock) void bn_apply_kernel(const bf16x8* __restrict__ x, const bf16x8* __restrict__ res,
                                                          bf16x8* __restrict__ y, const float* __restrict__ scale,
                                                          const float* __restrict__ bias, int64_t n_vec, int G,
                                                          uint8_t* __restrict__ mask, const float* __restrict__ rsb) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;  // multiple of G (G | 256 or G % 256 == 0 handled by host)
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_vec) return;
  const int cg = (int)(i % G);
  float a[8], b[8], ra[8], rb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = scale[cg * 8 + k];
    b[k] = bias[cg * 8 + k];
    ra[k] = 1.f;
    rb[k] = 0.f;
  }
  // rsb: the residual is the raw input of a BatchNorm (no activation) whose apply pass is deferred to here:
  // res' = res * rsb[c] + rsb[C + c]  (a ResNet downsampling branch feeds only this add)
  if (RES && rsb != nullptr) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ra[k] = rsb[cg * 8 + k];
      rb[k] = rsb[G * 8 + cg * 8 + k];
    }
  }
  for (; i < n_vec; i += stride) {
    const bf16x8 xv = x[i];
    bf16x8 rv;
    if constexpr (RES) rv = res[i];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = fmaf(bf2f(xv.v[k]), a[k], b[k]);
    if constexpr (RES) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += fmaf(bf2f(rv.v[k]), ra[k], rb[k]);
    }
    if constexpr (RELU) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
    }
    store8(y + i, v);
    if (RELU && mask != nullptr) {
      // ReLU mask, 1 bit per element (bit k of byte i = channel 8*cg+k of vector i): the backward reads this
      // 1/16-size tensor instead of y (a positive float stays positive after bf16 rounding, so bit == y > 0).
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) bits |= (uint32_t)(v[k] > 0.f) << k;
      mask[i] = (uint8_t)bits;
    }
  }
}

// ------------------------------------------------------------------------------- backward reduce
template <bool RELU>  // compile-time, so the mask load issues with the x / dy loads (see bn_apply_kernel)
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_kernel(const bf16x8* __restrict__ x, const uint8_t* __restrict__ mask,
                                                               const bf16x8* __restrict__ dy, int64_t M, int G, int Gb,
                                                               int64_t rows_per_block, const float* __restrict__ mean,
                                                               const float* __restrict__ invstd, int relu,
                                                               float* __restrict__ pdz, float* __restrict__ pdzx) {
  __shared__ float s_a[kBlock * 8];
  __shared__ float s_b[kBlock * 8];
  const int tid = threadIdx.x;
  const int cg_local = tid % Gb, rlane = tid / Gb, R = kBlock / Gb;
  const int cg = blockIdx.y * Gb + cg_local;
  const int C = G * 8;
  float mu[8], is[8], sa[8], sb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mu[k] = mean[cg * 8 + k];
    is[k] = invstd[cg * 8 + k];
    sa[k] = sb[k] = 0.f;
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > M) r1 = M;
#pragma unroll 4
  for (int64_t r = r0 + rlane; r < r1; r += R) {
    const int64_t off = r * G + cg;
    float xv[8], g[8];
    uint32_t mb = 0xffu;
    if constexpr (RELU) mb = mask[off];
    load8(x + off, xv);
    load8(dy + off, g);
    if constexpr (RELU) {
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = (mb >> k) & 1u ? g[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sa[k] += g[k];
      sb[k] = fmaf(g[k], (xv[k] - mu[k]) * is[k], sb[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    s_a[tid * 8 + k] = sa[k];
    s_b[tid * 8 + k] = sb[k];
  }
  __syncthreads();
  if (rlane == 0) {
    for (int j = 1; j < R; ++j) {
      const int o = (j * Gb + cg_local) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sa[k] += s_a[o + k];
        sb[k] += s_b[o + k];
      }
    }
    float* pa = pdz + (int64_t)blockIdx.x * C + cg * 8;
    float* pb = pdzx + (int64_t)blockIdx.x * C + cg * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pa[k] = sa[k];
      pb[k] = sb[k];
    }
  }
}

template <int NT>
__global__ __launch_bounds__(NT) void bn_bwd_finalize_kernel(const float* __restrict__ pdz, const float* __restrict__ pdzx, int nblk, int C,
                                       int64_t M, const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ invstd, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ coef, int accumulate) {
  double A, B;
  if (!fin_sum2<NT>(pdz, pdzx, nblk, C, A, B)) return;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const float db = (float)A, dg = (float)B;
  // accumulate: dgamma / dbeta are the parameters' own (flat) gradient slots, summed into like autograd would
  dbeta[c] = accumulate ? dbeta[c] + db : db;
  dgamma[c] = accumulate ? dgamma[c] + dg : dg;
  const float is = invstd[c], k1 = gamma[c] * is;
  const float k2 = db / (float)M, k3 = dg / (float)M;
  // dx = k1 * (dz - k2 - xhat*k3),  xhat = (x - mean) * is   =>  dx = A*dz + B*x + D
  coef[c] = k1;                                  // A
  coef[C + c] = -k1 * k3 * is;                   // B
  coef[2 * C + c] = -k1 * k2 + k1 * k3 * is * mean[c];  // D
}

// The BatchNorm that produced this one's residual input (a ResNet downsampling branch), when d_residual is that
// BatchNorm's complete gradient: the dx pass also reduces its per-block partials  sum dz2  and
// sum dz2 * (x2 - mean2) * invstd2  (dz2 = d_residual, masked by its own ReLU if it had one) into
// part[2][gridDim.x][C], so that BatchNorm's backward skips its reduce pass (plx_bn_backward with ext_part).
struct ResBn {
  const bf16x8* x;
  const uint8_t* mask;   // nullptr: no ReLU
  const float* mean;
  const float* invstd;
  float* part;           // nullptr: disabled
};

// RP: also reduce the residual BatchNorm's partials (ResBn).  A separate instantiation: its extra state
// (90 VGPRs) would cut the plain pass from 8 to 5 waves per SIMD, and this memory-bound pass needs them.
// RMASK (RP only): the residual BatchNorm had a ReLU (rb.mask set) -- compile-time, no per-trip pointer test
// DRES: d_residual = dz is stored (dres set) -- compile-time too: a consumer that takes (dy, mask) instead of dz
// (the downsample BatchNorm behind a ResBn, plx_gemm_nt_bndx) leaves the pass without the store and its pointer test
template <bool RP, bool RELU, bool RMASK, bool DRES>
__global__ __launch_bounds__(kBlock) void bn_bwd_dx_kernel(const bf16x8* __restrict__ x, const uint8_t* __restrict__ mask,
                                                           const bf16x8* __restrict__ dy, bf16x8* __restrict__ dx,
                                                           bf16x8* __restrict__ dres, const float* __restrict__ coef,
                                                           int64_t n_vec, int G, int relu, ResBn rb) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!RP && i >= n_vec) return;
  const int cg = (int)(i % G);  // fixed over the grid stride (grid * 256 % G == 0)
  const int C = G * 8;
  constexpr bool rp = RP;
  float A[8], B[8], D[8], mu2[8], is2[8], ra[8], rc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    A[k] = coef[cg * 8 + k];
    B[k] = coef[C + cg * 8 + k];
    D[k] = coef[2 * C + cg * 8 + k];
    ra[k] = rc[k] = 0.f;
    mu2[k] = rp ? rb.mean[cg * 8 + k] : 0.f;
    is2[k] = rp ? rb.invstd[cg * 8 + k] : 0.f;
  }
  for (; i < n_vec; i += stride) {
    float xv[8], g[8];
    uint32_t mb = 0xffu;
    if constexpr (RELU) mb = mask[i];  // issued with the x / dy loads (RELU is compile-time)
    load8(x + i, xv);
    load8(dy + i, g);
    if constexpr (RELU) {
#pragma unroll
      for (int k = 0; k < 8; ++k) g[k] = (mb >> k) & 1u ? g[k] : 0.f;
    }
    if constexpr (DRES) store8(dres + i, g);
    if constexpr (rp) {
      float x2[8];
      load8(rb.x + i, x2);
      const uint32_t m2 = RMASK ? rb.mask[i] : 0xffu;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float g2 = (m2 >> k) & 1u ? g[k] : 0.f;
        ra[k] += g2;
        rc[k] = fmaf(g2, (x2[k] - mu2[k]) * is2[k], rc[k]);
      }
    }
    float o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = fmaf(A[k], g[k], fmaf(B[k], xv[k], D[k]));
    store8(dx + i, o);
  }
  if constexpr (rp) {
  // threads tid, tid + G, ... of this block share channel group cg: sum them through LDS (G <= 256)
  __shared__ float red[kBlock * 16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[threadIdx.x * 16 + k] = ra[k];
    red[threadIdx.x * 16 + 8 + k] = rc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    for (int j = 1; j < kBlock / G; ++j) {
      const float* o = red + (j * G + threadIdx.x) * 16;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ra[k] += o[k];
        rc[k] += o[8 + k];
      }
    }
    float* pa = rb.part + (int64_t)blockIdx.x * C + cg * 8;
    float* pc = rb.part + ((int64_t)gridDim.x + blockIdx.x) * C + cg * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pa[k] = ra[k];
      pc[k] = rc[k];
    }
  }
  }
}

struct Plan {
  int G, Gb, gy, nblk, S;
  int64_t rows_per_block;
};

inline bool plan_for(int64_t M, int C, Plan* p) {
  if (M < 1 || C <= 0 || (C & 7)) return false;  // M < 1 first: rows_per_block would be 0, and nblk divides by it
  const int G = C / 8;
  if (G & (G - 1)) return false;  // power of two channel groups
  p->G = G;
  p->Gb = G < kBlock ? G : kBlock;
  p->gy = G / p->Gb;
  const int R = kBlock / p->Gb;
  const int64_t cap = (2048 + p->gy - 1) / p->gy;
  int64_t want = (M + 16 * R - 1) / (16 * R);  // every thread streams >= 16 rows
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  int64_t rpb = (M + want - 1) / want;
  rpb = (rpb + R - 1) / R * R;
  p->rows_per_block = rpb;
  p->nblk = (int)((M + rpb - 1) / rpb);
  p->S = (p->nblk + kRowsPerSplit - 1) / kRowsPerSplit;
  return true;
}

// grid-stride must keep each thread on one channel group: grid*256 % G == 0
inline int apply_grid(int64_t n_vec, int G) {
  int64_t g = (n_vec + kBlock - 1) / kBlock;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  const int64_t mult = G > kBlock ? G / kBlock : 1;
  g = (g + mult - 1) / mult * mult;
  return (int)g;
}

inline void launch_dx(hipStream_t stream, int64_t n_vec, int G, const void* x, const uint8_t* mask, const void* dy,
                      void* dx, void* dres, const float* coef, int relu, const ResBn& rb) {
  const dim3 grid(apply_grid(n_vec, G));
  auto pick = [&](auto d) {
    constexpr bool DRES = decltype(d)::value;
    return rb.part == nullptr
               ? (relu ? bn_bwd_dx_kernel<false, true, false, DRES> : bn_bwd_dx_kernel<false, false, false, DRES>)
           : rb.mask != nullptr
               ? (relu ? bn_bwd_dx_kernel<true, true, true, DRES> : bn_bwd_dx_kernel<true, false, true, DRES>)
               : (relu ? bn_bwd_dx_kernel<true, true, false, DRES> : bn_bwd_dx_kernel<true, false, false, DRES>);
  };
  auto k = dres != nullptr ? pick(std::true_type{}) : pick(std::false_type{});
  hipLaunchKernelGGL(k, grid, dim3(kBlock), 0, stream, (const bf16x8*)x, mask, (const bf16x8*)dy, (bf16x8*)dx,
                     (bf16x8*)dres, coef, n_vec, G, relu, rb);
}

inline void launch_apply(hipStream_t stream, int64_t n_vec, int G, const void* x, const void* res, void* y,
                         const float* scale, const float* bias, int relu, uint8_t* mask, const float* rsb) {
  auto k = res != nullptr ? (relu ? bn_apply_kernel<true, true> : bn_apply_kernel<true, false>)
                          : (relu ? bn_apply_kernel<false, true> : bn_apply_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(apply_grid(n_vec, G)), dim3(kBlock), 0, stream, (const bf16x8*)x, (const bf16x8*)res,
                     (bf16x8*)y, scale, bias, n_vec, G, mask, rsb);
}

// A/B knob (PLX_BN_FIN_SINGLE, plx_bn_set_fin_single): 1 = a one-launch reduce + finalize over at most kFinSingleMax
// partial rows runs in single workgroups (bn_*_finalize_single_kernel), 0 = every one takes the ticket kernels
int g_bn_fin_single = 1;

// Which kernels a reduce + finalize over nblk partial rows runs: 0 = reduce and finalize back to back (no counters),
// 1 = the ticket kernel, 2 = the single-workgroup kernel
enum { kFinTwoLaunch = 0, kFinTicket = 1, kFinSingle = 2 };

inline int fin_path(int nblk, int C, bool counters) {
  if (!counters) return kFinTwoLaunch;
  // the single kernel addresses the partials with 32-bit byte offsets: [2][nblk][C] floats below 2 GiB
  return g_bn_fin_single && nblk <= kFinSingleMax && (int64_t)nblk * C < (1 << 28) ? kFinSingle : kFinTicket;
}

// level-1 partials [2][nblk][C] -> finalize: one fused launch with a counter array (>= ceil(C/64) zeroed words; the
// single-workgroup kernel leaves it and the level-2 rows `l2` untouched), else the reduce and finalize kernels back
// to back
inline void reduce_finalize_fwd(hipStream_t stream, const float* part, int nblk, float* l2, unsigned* cnt,
                                const FwdFin& f) {
  const int C = f.C, S = (nblk + kRowsPerSplit - 1) / kRowsPerSplit;
  if (fin_path(nblk, C, cnt != nullptr) == kFinSingle) {
    // two splits (the 7x7 stage's 98 rows) or all eight in flight; 64 channels per workgroup
    auto k = S <= 2 ? bn_fwd_finalize_single_kernel<64, 2> : bn_fwd_finalize_single_kernel<64, kFinSingleSplits>;
    hipLaunchKernelGGL(k, dim3((C + 63) / 64), dim3(kFinNT), 0, stream, part, nblk, f);
    return;
  }
  if (cnt != nullptr) {
    hipLaunchKernelGGL(bn_fwd_reduce_finalize_kernel<kFinNT>, dim3((C + 63) / 64, S), dim3(kFinNT), 0, stream, part, nblk, l2, S,
                       cnt, f);
    return;
  }
  hipLaunchKernelGGL(bn_partial_reduce_kernel<kFinNT>,
                     dim3((C + 63) / 64, S, 2), dim3(kFinNT), 0, stream, part, nblk, C, l2, S);
  hipLaunchKernelGGL(bn_fwd_finalize_kernel<kFinNT>, dim3((C + 63) / 64),
                     dim3(kFinNT), 0, stream, l2, l2 + (int64_t)S * C, S,
                     f.x_row0, C, f.M, f.gamma, f.beta, f.eps, f.momentum, f.running_mean, f.running_var, f.save_mean,
                     f.save_invstd, f.scale, f.bias);
}

inline void reduce_finalize_bwd(hipStream_t stream, const float* part, int nblk, float* l2, unsigned* cnt,
                                const BwdFin& f) {
  const int C = f.C, S = (nblk + kRowsPerSplit - 1) / kRowsPerSplit;
  if (fin_path(nblk, C, cnt != nullptr) == kFinSingle) {
    // two splits (the 7x7 stage's 98 rows) or all eight in flight; 64 channels per workgroup
    auto k = S <= 2 ? bn_bwd_finalize_single_kernel<64, 2> : bn_bwd_finalize_single_kernel<64, kFinSingleSplits>;
    hipLaunchKernelGGL(k, dim3((C + 63) / 64), dim3(kFinNT), 0, stream, part, nblk, f);
    return;
  }
  if (cnt != nullptr) {
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel<kFinNT>, dim3((C + 63) / 64, S), dim3(kFinNT), 0, stream, part, nblk, l2, S,
                       cnt, f);
    return;
  }
  hipLaunchKernelGGL(bn_partial_reduce_kernel<kFinNT>,
                     dim3((C + 63) / 64, S, 2), dim3(kFinNT), 0, stream, part, nblk, C, l2, S);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<kFinNT>, dim3((C + 63) / 64),
                     dim3(kFinNT), 0, stream, l2, l2 + (int64_t)S * C, S, C,
                     f.M, f.gamma, f.mean, f.invstd, f.dgamma, f.dbeta, f.coef, f.accumulate);
}

// ------------------------------------------------------------------------------- ResNet stem: BN + ReLU + max-pool
// The stem's BatchNorm(+ReLU) output only feeds the 3x3/s2/p1 max-pool.  Forward: p = maxpool(bf16(relu(x*scale +
// bias))) in one pass over x with the window position (0..8) of each max (first max in (kh, kw) order, the rule of
// csrc/pool_kernels.hip), so the BatchNorm output (4x the pooled size) and its ReLU mask are never written or re-read.
// Backward: every input pixel gathers dy from the <= 2x2 windows whose argmax it is (maxpool_bwd_kernel's gather, the
// sum rounded to bf16 as that kernel stores it), masks it by the recomputed ReLU test (x*scale + bias > 0, the apply
// pass's test bit for bit) and either reduces the BatchNorm partials (pass 1) or writes dx = A*dz + B*x + D (pass 2):
// 2 passes over x instead of pool-bwd write + BN reduce + BN dx (3 reads and 2 writes of the 112x112 tensor).
struct alignas(8) u8x8 {
  uint8_t v[8];
};

__global__ __launch_bounds__(256) void stem_apply_pool_kernel(const bf16x8* __restrict__ x,
                                                              const float* __restrict__ sb, bf16x8* __restrict__ y,
                                                              u8x8* __restrict__ idx, int N, int H, int W, int G,
                                                              int OH, int OW) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= (unsigned)(OW * G)) return;
  const unsigned g = j % (unsigned)G, ow = j / (unsigned)G;
  const int C = G * 8;
  float a[8], b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = sb[g * 8 + k];
    b[k] = sb[C + g * 8 + k];
  }
  for (int row = blockIdx.y; row < N * OH; row += gridDim.y) {
    const int n = row / OH, oh = row - n * OH;
    float best[8];
    uint8_t arg[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      best[k] = -INFINITY;
      arg[k] = 255;
    }
    // all 9 window loads first, from clamped (always valid) addresses; out-of-image taps are skipped in the max
    // (a branch around each load made hipcc wait for every load before issuing the next)
    uint4 q[9];
    bool ok[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh * 2 - 1 + kh;
      const int ihc = ih < 0 ? 0 : (ih >= H ? H - 1 : ih);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = (int)ow * 2 - 1 + kw;
        const int iwc = iw < 0 ? 0 : (iw >= W ? W - 1 : iw);
        ok[kh * 3 + kw] = ih >= 0 && ih < H && iw >= 0 && iw < W;
        q[kh * 3 + kw] = *(const uint4*)(x + ((size_t)(n * H + ihc) * W + iwc) * G + g);
      }
    }
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
      const uint32_t qw[4] = {q[t9].x, q[t9].y, q[t9].z, q[t9].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xk = __uint_as_float((k & 1) ? (qw[k >> 1] & 0xffff0000u) : (qw[k >> 1] << 16));
        const float f = (float)(__bf16)fmaxf(fmaf(xk, a[k], b[k]), 0.f);  // the apply pass's bf16 value (RNE)
        if (ok[t9] && (f > best[k] || arg[k] == 255)) {
          best[k] = f;
          arg[k] = (uint8_t)t9;
        }
      }
    }
    bf16x8 o;
    u8x8 m;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o.v[k] = f2bf(best[k]);
      m.v[k] = arg[k];
    }
    const size_t t = (size_t)row * OW * G + j;
    y[t] = o;
    idx[t] = m;
  }
}

// input row / column i of a 3x3/s2/p1 pool is covered by output o = (i + 1 - k) / 2 for the taps k of matching parity
__device__ __forceinline__ int stem_cover(int i, int O, int* o, int* k) {
  int n = 0;
  if (i & 1) {
    if ((i + 1) >> 1 < O) { o[n] = (i + 1) >> 1; k[n++] = 0; }
    o[n] = (i - 1) >> 1; k[n++] = 2;
  } else if ((i >> 1) < O) {
    o[n] = i >> 1; k[n++] = 1;
  }
  return n;
}

// One thread = 8 channels of a 2x2 quad of input pixels (2a + di, 2b + dj): row 2a is covered only by output row a
// (tap kh = 1), row 2a + 1 by rows a (kh = 2) and a + 1 (kh = 0), likewise for columns, so the quad's gradient comes
// from the 4 windows (a + p, b + q) -- one window load per input pixel instead of every pixel gathering all 4 windows
// (a first per-pixel version ran 1.6x the unfused pool-bwd + BN-bwd time).  Grid (ceil(QW*G / 256), rows_y) over quad
// rows (n, a); block (bx, by) walks quad rows by, by + rows_y, ...  DX = false: per-block partials
// part[2][gridDim.x * gridDim.y][C] of sum dz and sum dz * xhat; DX = true: dx from coef = [A | B | D].
template <bool DX>
__global__ __launch_bounds__(256) void stem_pool_bn_bwd_kernel(const bf16x8* __restrict__ dy, const u8x8* __restrict__ idx,
                                                               const bf16x8* __restrict__ x, const float* __restrict__ sb,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ coef, bf16x8* __restrict__ dx,
                                                               float* __restrict__ part, int N, int H, int W, int G,
                                                               int OH, int OW) {
  const int QH = (H + 1) / 2, QW = (W + 1) / 2;
  const unsigned j0 = blockIdx.x * 256u + threadIdx.x;
  const bool active = j0 < (unsigned)(QW * G);
  const unsigned j = active ? j0 : 0u;
  const unsigned g = j % (unsigned)G;                     // == threadIdx.x % G (256 % G == 0)
  const int qb = (int)(j / (unsigned)G);
  const int C = G * 8;
  float a[8], b[8], c1[8], c2[8], c3[8], s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = sb[g * 8 + k];
    b[k] = sb[C + g * 8 + k];
    if constexpr (DX) {
      c1[k] = coef[g * 8 + k];
      c2[k] = coef[C + g * 8 + k];
      c3[k] = coef[2 * C + g * 8 + k];
    } else {
      c1[k] = mean[g * 8 + k];
      c2[k] = invstd[g * 8 + k];
      c3[k] = 0.f;
    }
    s1[k] = s2[k] = 0.f;
  }
  for (int row = blockIdx.y; active && row < N * QH; row += gridDim.y) {
    const int n = row / QH, qa = row - n * QH;
    // windows (qa + p, qb + q) and the quad's pixels: whole-vector loads from clamped addresses, all issued before
    // any use; validity is applied per element
    uint2 am[4];
    uint4 d[4], xq[4];
    bool wv[4], pv[4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int w4 = p * 2 + q, oh = qa + p, ow = qb + q;
        wv[w4] = oh < OH && ow < OW;
        const size_t off = ((size_t)(n * OH + (oh < OH ? oh : OH - 1)) * OW + (ow < OW ? ow : OW - 1)) * G + g;
        am[w4] = *(const uint2*)(idx + off);
        d[w4] = *(const uint4*)(dy + off);
        if (!wv[w4]) am[w4] = make_uint2(0xffffffffu, 0xffffffffu);  // no tap code (0..8) matches 0xff
        const int ih = 2 * qa + p, iw = 2 * qb + q;         // quad pixel (di, dj) = (p, q)
        pv[w4] = ih < H && iw < W;
        xq[w4] = *(const uint4*)(x + ((size_t)(n * H + (ih < H ? ih : H - 1)) * W + (iw < W ? iw : W - 1)) * G + g);
      }
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const int e = di * 2 + dj;
        const uint32_t xw[4] = {xq[e].x, xq[e].y, xq[e].z, xq[e].w};
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float acc = 0.f;
#pragma unroll
          for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const int kh = di + 1 - 2 * p, kw = dj + 1 - 2 * q;   // this pixel's tap in window (p, q)
              if (kh < 0 || kw < 0) continue;                      // compile-time
              const int w4 = p * 2 + q;
              const uint32_t ab = (k < 4 ? am[w4].x : am[w4].y) >> (8 * (k & 3)) & 0xffu;
              const uint32_t dw = (k >> 1) == 0 ? d[w4].x : (k >> 1) == 1 ? d[w4].y : (k >> 1) == 2 ? d[w4].z : d[w4].w;
              const float dv = __uint_as_float((k & 1) ? (dw & 0xffff0000u) : (dw << 16));
              acc += ab == (uint32_t)(kh * 3 + kw) ? dv : 0.f;   // invalid windows' bytes were set to 0xff
            }
          const float xf = __uint_as_float((k & 1) ? (xw[k >> 1] & 0xffff0000u) : (xw[k >> 1] << 16));
          // rounded to bf16 as the unfused pool backward stores it (a plain cast: one v_cvt_pk_bf16_f32, RNE)
          const float dz = (pv[e] && fmaf(xf, a[k], b[k]) > 0.f) ? (float)(__bf16)acc : 0.f;
          if constexpr (DX) {
            o[k] = fmaf(c1[k], dz, fmaf(c2[k], xf, c3[k]));
          } else {
            s1[k] += dz;
            s2[k] = fmaf(dz, (xf - c1[k]) * c2[k], s2[k]);
          }
        }
        if constexpr (DX) {
          if (pv[e]) store8(dx + ((size_t)(n * H + 2 * qa + di) * W + 2 * qb + dj) * G + g, o);
        }
      }
  }
  if constexpr (!DX) {
    // the 256 / G threads of this block that share channel group g: fixed-order sum through LDS
    __shared__ float red[256 * 17];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[threadIdx.x * 17 + k] = s1[k];
      red[threadIdx.x * 17 + 8 + k] = s2[k];
    }
    __syncthreads();
    const int nb = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
    for (int e = threadIdx.x; e < G * 16; e += 256) {     // e = (value v, group gg)
      const int gg = e % G, v = e / G;
      float sum = 0.f;
      for (int r = gg; r < 256; r += G) sum += red[r * 17 + v];
      const int c = gg * 8 + (v & 7);
      part[((int64_t)(v < 8 ? 0 : nb) + blk) * C + c] = sum;
    }
  }
}

// ---- thinned stem kernels (g_bn_thin): the same arithmetic per element as the three kernels above
// A/B knob (PLX_BN_THIN, plx_bn_set_thin): 1 = the thinned kernels serve the stem's forward / backward passes
// (stem_*_thin_kernel), 0 = their predecessors.  Both give bit-identical results.
int g_bn_thin = 1;

// Per-channel constants of the thinned kernels, staged once per block in LDS as float4 [array][half][group]: a thread
// reads the 4 channels (half h of its group's 8) of one array with one conflict-free 16-byte read (consecutive lanes,
// consecutive groups), just before it uses them, so no constant stays in a register across the loop.
__device__ __forceinline__ int thin_slot(int arr, int k, int grp, int ngrp) {
  return ((arr * 2 + (k >> 2)) * ngrp + grp) * 4 + (k & 3);
}

// Keeps the LDS reads of a loop trip inside the trip: hipcc would otherwise hoist them (loop invariant) and hold
// every constant in registers again.
__device__ __forceinline__ void thin_trip_fence() { asm volatile("" ::: "memory"); }

// Pins four registers at this point of the program: what is computed from them cannot move above it, what they
// were computed from cannot sink below it.
__device__ __forceinline__ void thin_pin4(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

// Keeps hipcc's scheduler from interleaving the channel pairs (or window taps) of a trip: each is scheduled on its
// own, in program order, so the temporaries of one are dead before the next begins.
__device__ __forceinline__ void thin_sched_fence() { __builtin_amdgcn_sched_barrier(0); }

constexpr int kStemFwdRows = 8;  // output rows a block of the thinned forward walks down
constexpr int kStemDxRows = 4;   // quad rows per block of the thinned dx pass

// bf16(relu(x * a + b)) of a pixel's 8 channels, packed as the apply pass would store them
__device__ __forceinline__ uint4 stem_tf(const uint4 q, const float* a, const float* b) {
  const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
  uint32_t r[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float lo = fmaxf(fmaf(__uint_as_float(qw[w] << 16), a[2 * w], b[2 * w]), 0.f);
    const float hi = fmaxf(fmaf(__uint_as_float(qw[w] & 0xffff0000u), a[2 * w + 1], b[2 * w + 1]), 0.f);
    r[w] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}

// one window tap of stem_apply_pool_kernel's max: `none` (no valid tap so far) is that kernel's arg[k] == 255,
// which is the same for all 8 channels, so it is kept once per thread
__device__ __forceinline__ void stem_tap(const uint4 f4, bool ok, bool& none, uint32_t t9, float* best, uint32_t* arg) {
  const uint32_t fw[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float f = __uint_as_float((k & 1) ? (fw[k >> 1] & 0xffff0000u) : (fw[k >> 1] << 16));
    if (ok && (f > best[k] || none)) {
      best[k] = f;
      arg[k] = t9;
    }
  }
  none = none && !ok;
  thin_sched_fence();
}

// stem_apply_pool_kernel with every input pixel transformed once per column of windows instead of once per window:
// a thread owns output column ow (8 channels) and walks down kStemFwdRows output rows of one image; input row
// 2 * oh + 1 is the last row of window oh and the first of window oh + 1, so its transformed values are carried over
// (6 loads and transforms per output instead of 9), and the next trip's loads are issued before this trip's math.
// Grid: gx * N * cpi blocks, gx = ceil(OW * G / 256) column chunks x cpi = ceil(OH / kStemFwdRows) row chunks per image.
__global__ __launch_bounds__(256) void stem_apply_pool_thin_kernel(const bf16x8* __restrict__ x,
                                                                   const float* __restrict__ sb,
                                                                   bf16x8* __restrict__ y, u8x8* __restrict__ idx,
                                                                   int H, int W, int G, int OH, int OW, int gx,
                                                                   int cpi) {
  const unsigned bx = blockIdx.x % (unsigned)gx, chunk = blockIdx.x / (unsigned)gx;
  const unsigned j = bx * 256u + threadIdx.x;
  if (j >= (unsigned)(OW * G)) return;
  const unsigned g = j % (unsigned)G, ow = j / (unsigned)G;
  const int C = G * 8;
  float a[8], b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = sb[g * 8 + k];
    b[k] = sb[C + g * 8 + k];
  }
  const int n = (int)chunk / cpi, oh0 = ((int)chunk - n * cpi) * kStemFwdRows;
  const int oh1 = oh0 + kStemFwdRows < OH ? oh0 + kStemFwdRows : OH;
  // the window's 3 columns: clamped (always valid) addresses, out-of-image taps are skipped in the max
  int col[3];
  bool cok[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int iw = (int)ow * 2 - 1 + kw;
    cok[kw] = iw >= 0 && iw < W;
    col[kw] = (iw < 0 ? 0 : (iw >= W ? W - 1 : iw)) * G;
  }
  const bf16x8* xn = x + (size_t)n * H * W * G + g;
  uint4 pr[3], q[6];  // transformed row 2 * oh - 1 (unused at oh = 0: never valid there); rows 2 * oh, 2 * oh + 1
  {
    const int ihp = oh0 > 0 ? 2 * oh0 - 1 : 0, ihb = 2 * oh0 + 1 < H ? 2 * oh0 + 1 : H - 1;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      pr[kw] = *(const uint4*)(xn + (size_t)ihp * W * G + col[kw]);
      q[kw] = *(const uint4*)(xn + (size_t)(2 * oh0) * W * G + col[kw]);
      q[3 + kw] = *(const uint4*)(xn + (size_t)ihb * W * G + col[kw]);
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) pr[kw] = stem_tf(pr[kw], a, b);
  }
  for (int oh = oh0; oh < oh1; ++oh) {
    uint4 nq[6];  // the next trip's rows (the last trip reloads its own)
    {
      const int ohn = oh + 1 < oh1 ? oh + 1 : oh, ihb = 2 * ohn + 1 < H ? 2 * ohn + 1 : H - 1;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        nq[kw] = *(const uint4*)(xn + (size_t)(2 * ohn) * W * G + col[kw]);
        nq[3 + kw] = *(const uint4*)(xn + (size_t)ihb * W * G + col[kw]);
      }
    }
    float best[8];
    uint32_t arg[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      best[k] = -INFINITY;
      arg[k] = 255;
    }
    bool none = true;
    const bool r0 = oh > 0, r2 = 2 * oh + 1 < H;  // row 2 * oh is always inside the image
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) stem_tap(pr[kw], r0 && cok[kw], none, kw, best, arg);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) stem_tap(stem_tf(q[kw], a, b), cok[kw], none, 3 + kw, best, arg);
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      pr[kw] = stem_tf(q[3 + kw], a, b);
      stem_tap(pr[kw], r2 && cok[kw], none, 6 + kw, best, arg);
    }
    bf16x8 o;
    u8x8 m;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o.v[k] = f2bf(best[k]);
      m.v[k] = (uint8_t)arg[k];
    }
    const size_t t = (size_t)(n * OH + oh) * OW * G + j;
    y[t] = o;
    idx[t] = m;
#pragma unroll
    for (int e = 0; e < 6; ++e) q[e] = nq[e];
  }
}

// stem_pool_bn_bwd_kernel<DX> with the per-channel constants in LDS (thin_slot: a | b | A | B | D for the dx pass,
// a | b | mean | invstd for the partials pass), read per half group (4 channels) right before their use, and the
// channels as the outer loop of a quad, so a quad's loads die half by half.  Per channel the 4 pixels are still taken
// in the order e = 0..3.  DX = false: the grid, the block -> quad-row assignment (by, by + rows_y, ...), each thread's
// accumulation order, the LDS sum and the partial layout are those of stem_pool_bn_bwd_kernel<false>.  DX = true:
// grid (ceil(QW * G / 256), ceil(rows / kStemDxRows)), a block takes kStemDxRows consecutive quad rows.
// Dynamic LDS: (DX ? 5 : 4) * C floats.
template <bool DX>
__global__ __launch_bounds__(256) void stem_pool_bn_bwd_thin_kernel(
    const bf16x8* __restrict__ dy, const u8x8* __restrict__ idx, const bf16x8* __restrict__ x,
    const float* __restrict__ sb, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ coef, bf16x8* __restrict__ dx, float* __restrict__ part, int N, int H, int W, int G,
    int OH, int OW) {
  extern __shared__ float4 thin_lds[];
  constexpr int NA = DX ? 5 : 4;
  const int QH = (H + 1) / 2, QW = (W + 1) / 2;
  const unsigned j0 = blockIdx.x * 256u + threadIdx.x;
  const bool active = j0 < (unsigned)(QW * G);
  const unsigned j = active ? j0 : 0u;
  const unsigned g = j % (unsigned)G;                     // == threadIdx.x % G (256 % G == 0)
  const int qb = (int)(j / (unsigned)G);
  const int C = G * 8;
  for (int e = threadIdx.x; e < NA * C; e += 256) {
    const int arr = e / C, c = e - arr * C;
    const float* src = arr == 0 ? sb : arr == 1 ? sb + C : DX ? coef + (arr - 2) * C : arr == 2 ? mean : invstd;
    ((float*)thin_lds)[thin_slot(arr, c & 7, c >> 3, G)] = src[c];
  }
  __syncthreads();
  float s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.f;
  const int rows = N * QH;
  const int row0 = DX ? blockIdx.y * kStemDxRows : blockIdx.y, step = DX ? 1 : gridDim.y;
  const int row1 = DX ? (row0 + kStemDxRows < rows ? row0 + kStemDxRows : rows) : rows;
  for (int row = row0; active && row < row1; row += step) {
    thin_trip_fence();
    const int n = row / QH, qa = row - n * QH;
    // windows (qa + p, qb + q) and the quad's pixels: whole-vector loads from clamped addresses, all issued before
    // any use; validity is applied per element
    uint2 am[4];
    uint4 d[4], xq[4];
    bool pv[4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int w4 = p * 2 + q, oh = qa + p, ow = qb + q;
        const size_t off = ((size_t)(n * OH + (oh < OH ? oh : OH - 1)) * OW + (ow < OW ? ow : OW - 1)) * G + g;
        am[w4] = *(const uint2*)(idx + off);
        d[w4] = *(const uint4*)(dy + off);
        if (!(oh < OH && ow < OW)) am[w4] = make_uint2(0xffffffffu, 0xffffffffu);  // no tap code (0..8) matches 0xff
        const int ih = 2 * qa + p, iw = 2 * qb + q;         // quad pixel (di, dj) = (p, q)
        pv[w4] = ih < H && iw < W;
        xq[w4] = *(const uint4*)(x + ((size_t)(n * H + (ih < H ? ih : H - 1)) * W + (iw < W ? iw : W - 1)) * G + g);
      }
    uint32_t amw[4][2], dw[4][4], xw[4][4];
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) {
      amw[w4][0] = am[w4].x, amw[w4][1] = am[w4].y;
      dw[w4][0] = d[w4].x, dw[w4][1] = d[w4].y, dw[w4][2] = d[w4].z, dw[w4][3] = d[w4].w;
      xw[w4][0] = xq[w4].x, xw[w4][1] = xq[w4].y, xw[w4][2] = xq[w4].z, xw[w4][3] = xq[w4].w;
    }
    uint32_t ow4[4][4];  // dx of the quad's 4 pixels, packed
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float cst[NA][4];
#pragma unroll
      for (int arr = 0; arr < NA; ++arr) {
        const float4 v = thin_lds[(arr * 2 + h) * G + g];
        cst[arr][0] = v.x, cst[arr][1] = v.y, cst[arr][2] = v.z, cst[arr][3] = v.w;
      }
      thin_pin4(amw[0][h], amw[1][h], amw[2][h], amw[3][h]);
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {  // a channel pair = one register of every load
        const int w = h * 2 + kp;
        thin_pin4(dw[0][w], dw[1][w], dw[2][w], dw[3][w]);
        thin_pin4(xw[0][w], xw[1][w], xw[2][w], xw[3][w]);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int kk = kp * 2 + k2, k = h * 4 + kk;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int di = e >> 1, dj = e & 1;
            float acc = 0.f;
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
              for (int q = 0; q < 2; ++q) {
                const int kh = di + 1 - 2 * p, kw = dj + 1 - 2 * q;   // this pixel's tap in window (p, q)
                if (kh < 0 || kw < 0) continue;                      // compile-time
                const int w4 = p * 2 + q;
                const uint32_t ab = amw[w4][h] >> (8 * kk) & 0xffu;
                const float dv = __uint_as_float(k2 ? (dw[w4][w] & 0xffff0000u) : (dw[w4][w] << 16));
                acc += ab == (uint32_t)(kh * 3 + kw) ? dv : 0.f;   // invalid windows' bytes were set to 0xff
              }
            const float xf = __uint_as_float(k2 ? (xw[e][w] & 0xffff0000u) : (xw[e][w] << 16));
            // rounded to bf16 as the unfused pool backward stores it (a plain cast: one v_cvt_pk_bf16_f32, RNE)
            const float dz = (pv[e] && fmaf(xf, cst[0][kk], cst[1][kk]) > 0.f) ? (float)(__bf16)acc : 0.f;
            if constexpr (DX) {
              const uint32_t ob = f2bf(fmaf(cst[2][kk], dz, fmaf(cst[3][kk], xf, cst[NA - 1][kk])));
              ow4[e][w] = k2 ? (ow4[e][w] | (ob << 16)) : ob;
            } else {
              s1[k] += dz;
              s2[k] = fmaf(dz, (xf - cst[2][kk]) * cst[3][kk], s2[k]);
            }
          }
        }
        if constexpr (DX) thin_pin4(ow4[0][w], ow4[1][w], ow4[2][w], ow4[3][w]);  // formed here, not at the stores
        thin_sched_fence();
      }
    }
    if constexpr (DX) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (pv[e])
          *(uint4*)(dx + ((size_t)(n * H + 2 * qa + (e >> 1)) * W + 2 * qb + (e & 1)) * G + g) =
              make_uint4(ow4[e][0], ow4[e][1], ow4[e][2], ow4[e][3]);
    }
  }
  if constexpr (!DX) {
    // the 256 / G threads of this block that share channel group g: fixed-order sum through LDS
    __shared__ float red[256 * 17];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[threadIdx.x * 17 + k] = s1[k];
      red[threadIdx.x * 17 + 8 + k] = s2[k];
    }
    __syncthreads();
    const int nb = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
    for (int e = threadIdx.x; e < G * 16; e += 256) {     // e = (value v, group gg)
      const int gg = e % G, v = e / G;
      float sum = 0.f;
      for (int r = gg; r < 256; r += G) sum += red[r * 17 + v];
      const int c = gg * 8 + (v & 7);
      part[((int64_t)(v < 8 ? 0 : nb) + blk) * C + c] = sum;
    }
  }
}

// over quad rows: pass 1 (partials) a few per block (rows_y <= g_stem_bwd_cap bounds the level-1 partials: 4096 rows
// ~4 MB at the stem's shape), pass 2 (dx) one per block.
constexpr int g_stem_bwd_cap = 4096;

inline dim3 stem_bwd_grid(int N, int H, int W, int G, bool dx) {
  const int rows = N * ((H + 1) / 2), cap = dx ? 65535 : g_stem_bwd_cap;
  return dim3((((W + 1) / 2) * G + 255) / 256, rows < cap ? rows : cap);
}

}  // namespace

// A/B knob: 1 (default) = the thinned stem kernels, 0 = their predecessors (g_bn_thin)
PLX_API void plx_bn_set_thin(int on) { g_bn_thin = on != 0; }

// A/B knob: 1 (default) = single-workgroup reduce + finalize for few partial rows, 0 = the ticket kernels throughout
PLX_API void plx_bn_set_fin_single(int on) { g_bn_fin_single = on != 0; }

// Host only: the kernels that the reduce + finalize of a call WITH a counter array runs for nblk partial rows of C
// channels under the current switch: 1 = the ticket kernel, 2 = the single-workgroup kernel (-1: not a valid call).
// A call without counters always runs the reduce and the finalize kernel back to back.
PLX_API int plx_bn_fin_path(int nblk, int C) {
  if (nblk < 1 || C < 8 || C % 8 || ((C / 8) & (C / 8 - 1))) return -1;
  return fin_path(nblk, C, true);
}

// fp32 workspace of a call that runs its own statistics / reduce pass: level-1 [2][nblk][C] + level-2 [2][S][C].
PLX_API int64_t plx_bn_workspace(int64_t M, int C) {
  Plan p;
  if (!plan_for(M, C, &p)) return -1;
  return 2 * (int64_t)(p.nblk + p.S) * C;
}

// fp32 workspace of a call that is given level-1 partials ([2][nblk][C], e.g. from the 1x1-conv GEMM epilogue,
// csrc/conv_gemm.hip): the level-2 rows only, 2 * ceil(nblk / 64) * C floats.
PLX_API int64_t plx_bn_l2_workspace(int nblk, int C) {
  return 2 * (int64_t)((nblk + kRowsPerSplit - 1) / kRowsPerSplit) * C;
}

// Row blocks of the dx pass = the nblk of the residual-BatchNorm partials it writes (ResBn).
PLX_API int plx_bn_dx_blocks(int64_t M, int C) {
  Plan p;
  if (!plan_for(M, C, &p)) return -1;
  return apply_grid(M * p.G, p.G);
}

// Arguments of plx_bn_forward / plx_bn_backward (host images: ops/_native.py BnForwardArgs / BnBackwardArgs, their
// sizes compared with plx_bn_args_size at load).  Common to both:
//   ext_part == nullptr: the call runs its own statistics / reduce pass over x into `workspace`
//                        (plx_bn_workspace(M, C) floats)
//   ext_part given:      level-1 partials [2][ext_nblk][C] from the op that wrote x (forward: unshifted sum, sum of
//                        squares) or dy (backward: sum dz, sum dz*xhat); no pass over x, and `workspace` holds only
//                        the level-2 rows (plx_bn_l2_workspace(ext_nblk, C) floats)
//   counters (nullable): >= ceil(C/64) zeroed words, reduce + finalize then run as one launch
struct BnForwardArgs {
  const void *x, *res;    // res nullable: residual added before the activation
  void* y;                // nullptr: statistics and scale/bias only (the apply is deferred to the consumer)
  int64_t M;
  int C, relu;
  const float *gamma, *beta;
  float eps, momentum;
  float *running_mean, *running_var;  // nullable (both)
  float *save_mean, *save_invstd, *scale_bias /* [2C] */, *workspace;
  const float* ext_part;
  int ext_nblk;
  uint8_t* mask;          // M*C/8 bytes, written when relu (nullable: no mask wanted)
  const float* res_sb;    // nullable [2C], see bn_apply_kernel
  unsigned* counters;
};

struct BnBackwardArgs {
  const void* x;
  const uint8_t* mask;    // the ReLU bit mask dz = dy * mask is formed with: required when relu and a pass reads it.
                          // The forward's own, or a foreign one: that of the ReLU downstream whose incoming gradient dy
                          // is (a downsample BatchNorm behind bn3's add + ReLU, handed bn3's dy instead of d_residual)
  const void* dy;
  void* dx;               // nullptr: reduce + finalize only (dgamma, dbeta, coef): dx = coef[0] * dz + coef[1] * x +
                          // coef[2] is then formed by the data-gradient GEMM that consumes it (plx_gemm_nt_bndx)
  void* dres;             // nullable: d_residual = dz, written by the dx pass
  int64_t M;
  int C, relu;
  const float *gamma, *save_mean, *save_invstd;
  float *dgamma, *dbeta, *coef /* [3C] */, *workspace;
  const float* ext_part;
  int ext_nblk, accumulate;  // accumulate: dgamma / dbeta += (else =)
  ResBn resbn;            // all null: none; else needs dx, C <= 2048, and dres unless no_dres
  unsigned* counters;
  int no_dres;            // 1: the caller states that d_residual's consumer takes (dy, mask) instead of dz, so a ResBn
                          // comes without dres (0: a ResBn without dres is a forgotten buffer and is refused)
};

PLX_API int plx_bn_args_size(int backward) {
  return (int)(backward ? sizeof(BnBackwardArgs) : sizeof(BnForwardArgs));
}

PLX_API int plx_bn_forward(const BnForwardArgs* a, hipStream_t stream) {
  Plan p;
  const int C = a->C;
  if (!plan_for(a->M, C, &p) || (a->ext_part != nullptr && a->ext_nblk < 1)) return 1;
  const bool own = a->ext_part == nullptr;  // this call runs the statistics pass itself
  const int nblk = own ? p.nblk : a->ext_nblk;
  float* l2 = own ? a->workspace + 2 * (int64_t)nblk * C : a->workspace;
  if (own)
    hipLaunchKernelGGL(bn_stats_kernel, dim3(p.nblk, p.gy), dim3(kBlock), 0, stream, (const bf16x8*)a->x, a->M, p.G,
                       p.Gb, p.rows_per_block, a->workspace, a->workspace + (int64_t)nblk * C);
  // x_row0: the own pass sums x shifted by its first row; external partials are unshifted sums
  reduce_finalize_fwd(stream, own ? a->workspace : a->ext_part, nblk, l2, a->counters,
                      FwdFin{own ? (const uint16_t*)a->x : nullptr, C, a->M, a->gamma, a->beta, a->eps, a->momentum, a->running_mean,
                             a->running_var, a->save_mean, a->save_invstd, a->scale_bias, a->scale_bias + C});
  if (a->y != nullptr)
    launch_apply(stream, a->M * p.G, p.G, a->x, a->res, a->y, a->scale_bias, a->scale_bias + C, a->relu,
                 a->relu ? a->mask : nullptr, a->res_sb);
  return (int)hipGetLastError();
}

PLX_API int plx_bn_backward(const BnBackwardArgs* a, hipStream_t stream) {
  Plan p;
  const int C = a->C, relu = a->relu;
  const ResBn& rb = a->resbn;
  const bool has_rb = rb.x != nullptr || rb.mask != nullptr || rb.mean != nullptr || rb.invstd != nullptr ||
                      rb.part != nullptr;
  if (!plan_for(a->M, C, &p) || (a->ext_part != nullptr && a->ext_nblk < 1)) return 1;
  // the reduce and the dx pass read the mask; with external partials and no dx pass nothing does
  if (relu && a->mask == nullptr && (a->ext_part == nullptr || a->dx != nullptr)) return 1;
  // a ResBn needs the dx pass (below); dres too, unless the caller states that d_residual's consumer takes (dy, mask)
  // instead of dz (no_dres) -- and then passing one is a contradiction
  if (has_rb && (rb.part == nullptr || rb.x == nullptr || rb.mean == nullptr || rb.invstd == nullptr)) return 1;
  if (has_rb && (a->dres == nullptr) != (a->no_dres != 0)) return 1;
  if (!has_rb && a->no_dres) return 1;
  if (a->dx == nullptr && (a->dres != nullptr || has_rb)) return 1;
  // the dx pass sums a ResBn's partials over the threads of ONE block that share a channel group: above kBlock groups
  // (C > 2048) a block holds only kBlock of the G groups of a row of `part` and would leave the others unwritten
  if (has_rb && p.G > kBlock) return 1;
  const bool own = a->ext_part == nullptr;  // this call runs the reduce pass itself
  const int nblk = own ? p.nblk : a->ext_nblk;
  float* l2 = own ? a->workspace + 2 * (int64_t)nblk * C : a->workspace;
  if (own)
    hipLaunchKernelGGL(relu ? bn_bwd_reduce_kernel<true> : bn_bwd_reduce_kernel<false>, dim3(p.nblk, p.gy),
                       dim3(kBlock), 0, stream, (const bf16x8*)a->x, a->mask, (const bf16x8*)a->dy, a->M, p.G, p.Gb,
                       p.rows_per_block, a->save_mean, a->save_invstd, relu, a->workspace,
                       a->workspace + (int64_t)nblk * C);
  reduce_finalize_bwd(stream, own ? a->workspace : a->ext_part, nblk, l2, a->counters,
                      BwdFin{C, a->M, a->gamma, a->save_mean, a->save_invstd, a->dgamma, a->dbeta, a->coef,
                             a->accumulate});
  if (a->dx != nullptr) launch_dx(stream, a->M * p.G, p.G, a->x, a->mask, a->dy, a->dx, a->dres, a->coef, relu, rb);
  return (int)hipGetLastError();
}

PLX_API int plx_bn_apply(const void* x, const void* res, void* y, int64_t M, int C, const float* scale_bias, int relu,
                         hipStream_t stream) {
  Plan p;
  if (!plan_for(M, C, &p)) return 1;
  const int64_t n_vec = M * p.G;
  launch_apply(stream, n_vec, p.G, x, res, y, scale_bias, scale_bias + C, relu, nullptr, nullptr);
  return (int)hipGetLastError();
}

// The training forward's apply + residual + ReLU pass on its own (bn_apply_kernel<true, true>): y and the 1-bit mask
// from scale_bias, with res_sb (nullable [2C]) the residual's deferred affine.  It fills a block output whose apply was
// deferred to a consumer that did not take it (ops/conv1x1.py PendingApply), and is what plx_gemm_nt_bnapply is
// tested against.
PLX_API int plx_bn_apply_res_relu(const void* x, const void* res, void* y, int64_t M, int C, const float* scale_bias,
                                  uint8_t* mask, const float* res_sb, hipStream_t stream) {
  Plan p;
  if (!plan_for(M, C, &p) || M < 1 || res == nullptr || mask == nullptr) return 1;
  launch_apply(stream, M * p.G, p.G, x, res, y, scale_bias, scale_bias + C, 1, mask, res_sb);
  return (int)hipGetLastError();
}

// ---- ResNet stem BatchNorm + ReLU + 3x3/s2/p1 max-pool (see stem_apply_pool_kernel)
// Forward: statistics (workspace `partials`: plx_bn_workspace(N*H*W, C) floats) -> mean / invstd / scale|bias ->
// y [N][OH][OW][C] bf16 and idx [N*OH*OW*C] window positions.
// ext_part / ext_nblk (nullable / 0): level-1 channel-stat partials [2][ext_nblk][C] from the producing convolution's
// epilogue (plx_stem_conv_fwd); `partials` then only needs the level-2 rows (plx_bn_l2_workspace(ext_nblk, C))
PLX_API int plx_stem_bn_pool_forward(const void* x, void* y, void* idx, int N, int H, int W, int C, const float* gamma,
                                     const float* beta, float eps, float momentum, float* running_mean,
                                     float* running_var, float* save_mean, float* save_invstd, float* scale_bias,
                                     float* partials, const float* ext_part, int ext_nblk, unsigned* counters,
                                     hipStream_t stream) {
  const int G = C / 8;
  if (N <= 0 || H <= 0 || W <= 0 || C % 8 || G > 256 || 256 % G) return 1;
  // statistics and scale/bias only: no res, y or mask
  const BnForwardArgs a{x, nullptr, nullptr, (int64_t)N * H * W, C, /*relu*/ 1, gamma, beta, eps, momentum,
                        running_mean, running_var, save_mean, save_invstd, scale_bias, partials, ext_part, ext_nblk,
                        /*mask*/ nullptr, /*res_sb*/ nullptr, counters};
  const int rc = plx_bn_forward(&a, stream);
  if (rc) return rc;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int rows = N * OH;
  if (g_bn_thin) {
    const int gx = (OW * G + 255) / 256, cpi = (OH + kStemFwdRows - 1) / kStemFwdRows;
    if ((int64_t)gx * N * cpi > 0x7fffffff) return 1;
    hipLaunchKernelGGL(stem_apply_pool_thin_kernel, dim3(gx * N * cpi), dim3(256), 0, stream, (const bf16x8*)x,
                       scale_bias, (bf16x8*)y, (u8x8*)idx, H, W, G, OH, OW, gx, cpi);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(stem_apply_pool_kernel, dim3((OW * G + 255) / 256, rows < 65535 ? rows : 65535), dim3(256), 0,
                     stream, (const bf16x8*)x, scale_bias, (bf16x8*)y, (u8x8*)idx, N, H, W, G, OH, OW);
  return (int)hipGetLastError();
}

// floats of workspace plx_stem_bn_pool_backward needs: level-1 [2][nblk][C] + level-2 [2][S][C]
PLX_API int64_t plx_stem_bn_pool_bwd_workspace(int N, int H, int W, int C) {
  const dim3 g = stem_bwd_grid(N, H, W, C / 8, false);
  const int64_t nblk = (int64_t)g.x * g.y;
  return 2 * (nblk + (nblk + kRowsPerSplit - 1) / kRowsPerSplit) * C;
}

// dy: gradient of the pooled output; dx: gradient of the BatchNorm input x.  dgamma / dbeta (+)= with accumulate.
PLX_API int plx_stem_bn_pool_backward(const void* dy, const void* idx, const void* x, void* dx, int N, int H, int W,
                                      int C, const float* gamma, const float* save_mean, const float* save_invstd,
                                      const float* scale_bias, float* dgamma, float* dbeta, float* coef,
                                      float* workspace, int accumulate, unsigned* counters, hipStream_t stream) {
  const int G = C / 8;
  if (N <= 0 || H <= 0 || W <= 0 || C % 8 || G > 256 || 256 % G) return 1;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const dim3 grid = stem_bwd_grid(N, H, W, G, false), grid_dx = stem_bwd_grid(N, H, W, G, true);
  const int nblk = grid.x * grid.y;
  if (g_bn_thin) {
    const int rows = N * ((H + 1) / 2);
    const dim3 grid_thin(grid.x, (rows + kStemDxRows - 1) / kStemDxRows);
    hipLaunchKernelGGL(stem_pool_bn_bwd_thin_kernel<false>, grid, dim3(256), sizeof(float) * 4 * C, stream,
                       (const bf16x8*)dy, (const u8x8*)idx, (const bf16x8*)x, scale_bias, save_mean, save_invstd,
                       (const float*)nullptr, (bf16x8*)nullptr, workspace, N, H, W, G, OH, OW);
    reduce_finalize_bwd(stream, workspace, nblk, workspace + 2 * (int64_t)nblk * C, counters,
                        BwdFin{C, (int64_t)N * H * W, gamma, save_mean, save_invstd, dgamma, dbeta, coef, accumulate});
    if (grid_thin.y <= 65535)
      hipLaunchKernelGGL(stem_pool_bn_bwd_thin_kernel<true>, grid_thin, dim3(256), sizeof(float) * 5 * C, stream,
                         (const bf16x8*)dy, (const u8x8*)idx, (const bf16x8*)x, scale_bias, save_mean, save_invstd,
                         coef, (bf16x8*)dx, (float*)nullptr, N, H, W, G, OH, OW);
    else  // more quad-row chunks than a grid's y extent: the predecessor loops over rows
      hipLaunchKernelGGL(stem_pool_bn_bwd_kernel<true>, grid_dx, dim3(256), 0, stream, (const bf16x8*)dy,
                         (const u8x8*)idx, (const bf16x8*)x, scale_bias, save_mean, save_invstd, coef, (bf16x8*)dx,
                         (float*)nullptr, N, H, W, G, OH, OW);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(stem_pool_bn_bwd_kernel<false>, grid, dim3(256), 0, stream, (const bf16x8*)dy, (const u8x8*)idx,
                     (const bf16x8*)x, scale_bias, save_mean, save_invstd, (const float*)nullptr, (bf16x8*)nullptr,
                     workspace, N, H, W, G, OH, OW);
  reduce_finalize_bwd(stream, workspace, nblk, workspace + 2 * (int64_t)nblk * C, counters,
                      BwdFin{C, (int64_t)N * H * W, gamma, save_mean, save_invstd, dgamma, dbeta, coef, accumulate});
  hipLaunchKernelGGL(stem_pool_bn_bwd_kernel<true>, grid_dx, dim3(256), 0, stream, (const bf16x8*)dy, (const u8x8*)idx,
                     (const bf16x8*)x, scale_bias, save_mean, save_invstd, coef, (bf16x8*)dx, (float*)nullptr, N, H,
                     W, G, OH, OW);
  return (int)hipGetLastError();
}
