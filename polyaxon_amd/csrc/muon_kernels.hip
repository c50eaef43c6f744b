// Muon on the flat parameter buffer for MI355X (gfx950): momentum, then five Newton-Schulz iterations on every
// selected weight matrix, batched over the whole model.
//
// For a matrix U (r rows, c columns, row-major, m = min(r, c)) the iteration orthogonalises X = U (r <= c) or X = U^T
// (r > c), X m x n:      A = X X^T      B = b A + c A A      X' = a X + B X          (a, b, c) below, five times.
// Operands are bf16, accumulation is fp32, and X, A, B are stored as bf16 in a workspace.
//
//   plx_muon_momentum   chunks that never cross a matrix: m <- mu m + g, u = g + mu m, u stored as bf16 in the
//                       matrix's own row-major layout, the gradient zeroed, one sum of squares per chunk.
//   plx_muon_norms      one wave per matrix sums its chunks in chunk order: scale = 1 / (|u| + 1e-7).
//   plx_muon_stage      one launch per stage over a host-built tile table (problem, tile row, tile column): every
//                       matrix of the model in one grid.  The normalisation is not a pass: X0 = scale u only ever
//                       appears as the first iteration's epilogue scalars (scale^2 on A, scale on X'), so u is
//                       rounded to bf16 once, unscaled.
//   plx_muon_update     w <- w (1 - lr_m wd) - lr_m sqrt(max(1, r / c)) O over the same chunks.
//
// The batched GEMM.  128 x 128 output tiles, K steps of 64, four waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16_bf16
// accumulators each).  Global loads are 16 bytes under a bounds predicate (every dimension is a multiple of 8, so a
// vector is inside or outside as a whole; outside reads nothing and stages zeros), held in registers over the MFMAs
// of the current K step and then written to the other of two LDS stages: one barrier per K step.
//
// A tall matrix is never transposed in memory: orientation is a property of the operand.  An operand is either
// K-contiguous (image [128][64], fragments by 16-byte LDS reads) or K-strided (image [64][128], fragments by
// ds_read_b64_tr_b16).  The transposing read delivers k in the order 8 (j >> 2) + 4 h + (j & 3) (h: the lane's half),
// so a K-contiguous operand paired with a K-strided one is read in that order too (two 8-byte reads).
//
//                 r <= c (X = U)                         r > c (X = U^T)
//   stage 1  A = U U^T      both K-contiguous        A = U^T U      both K-strided
//   stage 2  B = bA + cAA^T both K-contiguous        the same (A is symmetric, so A A = A A^T)
//   stage 3  U' = aU + B U  B K-contiguous,          U' = aU + U B^T both K-contiguous (B is symmetric)
//                           U K-strided
//
// Stages 1 and 2 list only tiles with column >= row and write the mirrored tile from the same accumulators (of a
// diagonal tile: the elements above the diagonal), so A and B are symmetric bit for bit and a quarter to a third of
// the iteration's MFMAs are never issued.
//
// Nothing is atomic and every sum has a fixed order.  `state` (optional) is the clip state of train_kernels.hip: the
// gradient is multiplied by state[1] as a rounding step of its own, and state[3] != 0 (skipped step) leaves momentum
// and weights alone: only the gradients are zeroed.
//
// hp: AdamW's (train_kernels.hip) with [4] weight_decay [6] muon_lr [7] muon_momentum.  sched (optional): the LR
// schedule's tensor; lr_m = hp[6] hp[0] / sched[0] when sched[0] > 0, so the schedule's factor reaches muon_lr.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLX_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr float kA = 3.4445f, kB = -4.7750f, kC = 2.0315f;

constexpr int kBlock = 256;
constexpr int kChunk = 16384;  // elements per chunk of the momentum / update passes
constexpr int kGridCap = 4096;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int PITCH_KC = 144;          // bytes per row of a K-contiguous image: 64 bf16 + 16
constexpr int PITCH_KS = 272;          // bytes per row of a K-strided image: 128 bf16 + 16
constexpr int IMG = BM * PITCH_KC;     // 18432 >= BK * PITCH_KS (17408)
constexpr int kSmem = 4 * IMG;         // two stages of an A and a B image

typedef unsigned short u16;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef u16 u16x4 __attribute__((ext_vector_type(4)));

// Per matrix: where its X (two buffers: an iteration reads one and writes the other), A and B live in the workspace
// (bf16 elements, multiples of 8), its shape and its first flat element.
struct Problem {
  int64_t x[2], a, b;
  int64_t rows, cols;
  int64_t flat, pad;
};

struct Tile {
  int problem, ti, tj, pad;
};

__device__ __forceinline__ float bf16_to_f(u16 h) { return __uint_as_float((uint32_t)h << 16); }

__device__ __forceinline__ u16 f_to_bf16(float f) {  // hardware RNE conversion (v_cvt_pk_bf16_f32)
  return __builtin_bit_cast(u16, (__bf16)f);
}

// ---------------------------------------------------------------- GEMM: staging
// The 16-byte vectors of this thread for one K step of one operand.  K-contiguous: operand(i, k) = p[i * ld + k];
// K-strided: operand(i, k) = p[k * ld + i].  i < R and k < K bound the reads.
template <bool KS>
__device__ __forceinline__ void load_global(const u16* __restrict__ p, int64_t ld, int R, int K, int i0, int k0,
                                            uint4 (&v)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = threadIdx.x + kBlock * q;
    int i, k;
    if constexpr (KS) {
      k = k0 + (e >> 4), i = i0 + ((e & 15) << 3);
    } else {
      i = i0 + (e >> 3), k = k0 + ((e & 7) << 3);
    }
    v[q] = make_uint4(0, 0, 0, 0);
    if (i < R && k < K) v[q] = *reinterpret_cast<const uint4*>(p + (KS ? (int64_t)k * ld + i : (int64_t)i * ld + k));
  }
}

template <bool KS>
__device__ __forceinline__ void store_lds(char* img, const uint4 (&v)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = threadIdx.x + kBlock * q;
    const int off = KS ? (e >> 4) * PITCH_KS + ((e & 15) << 4) : (e >> 3) * PITCH_KC + ((e & 7) << 4);
    *reinterpret_cast<uint4*>(img + off) = v[q];
  }
}

// ---------------------------------------------------------------- GEMM: fragments of the 32 operand rows at i0, k
// step kk (16 wide).  Lane l holds row l & 31; natural order: k = 16 kk + 8 h + j; transposed order (`PERM`, and every
// K-strided image): k = 16 kk + 8 (j >> 2) + 4 h + (j & 3).
template <bool PERM>
__device__ __forceinline__ bf16x8 frag_kc(const char* img, int i0, int kk, int lane) {
  const int h = lane >> 5;
  const char* row = img + (i0 + (lane & 31)) * PITCH_KC + kk * 32;
  if constexpr (PERM) {
    const s16x4 a = *reinterpret_cast<const s16x4*>(row + 8 * h);
    const s16x4 b = *reinterpret_cast<const s16x4*>(row + 16 + 8 * h);
    const s16x8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, r);
  } else {
    return *reinterpret_cast<const bf16x8*>(row + 16 * h);
  }
}

__device__ __forceinline__ s16x4 tr4(const char* img, int k, int i) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(img + k * PITCH_KS + i * 2));
}

// Each group of 16 lanes hands the instruction a 4 (k) x 16 (i) block and gets it back transposed: lane l receives
// rows k .. k + 3 of column i0 + (l & 31).
__device__ __forceinline__ bf16x8 frag_ks(const char* img, int i0, int kk, int lane) {
  const int h = lane >> 5, g1 = (lane >> 4) & 1, i = lane & 15;
  const int k = 16 * kk + 4 * h + (i >> 2);
  const int col = i0 + 16 * g1 + 4 * (i & 3);
  const s16x4 a = tr4(img, k, col), b = tr4(img, k + 8, col);
  const s16x8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, r);
}

template <bool KS, bool PERM>
__device__ __forceinline__ bf16x8 frag(const char* img, int i0, int kk, int lane) {
  if constexpr (KS) return frag_ks(img, i0, kk, lane);
  else return frag_kc<PERM>(img, i0, kk, lane);
}

// acc[tm][tn] += the wave's 64 x 64 part of opA(m0.., :) opB(:, n0..) over all of K.
template <bool AKS, bool BKS>
__device__ __forceinline__ void gemm_tile(const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B,
                                          int64_t ldb, int M, int N, int K, int m0, int n0, char* smem,
                                          f32x16 (&acc)[2][2]) {
  constexpr bool PERM = AKS || BKS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  uint4 va[4], vb[4];
  const int nk = (K + BK - 1) / BK;
  load_global<AKS>(A, lda, M, K, m0, 0, va);
  load_global<BKS>(B, ldb, N, K, n0, 0, vb);
  store_lds<AKS>(smem, va);
  store_lds<BKS>(smem + IMG, vb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* ia = smem + (kt & 1) * 2 * IMG;
    const char* ib = ia + IMG;
    if (kt + 1 < nk) {
      load_global<AKS>(A, lda, M, K, m0, (kt + 1) * BK, va);
      load_global<BKS>(B, ldb, N, K, n0, (kt + 1) * BK, vb);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = frag<AKS, PERM>(ia, wm + 32 * t, kk, lane);
        fb[t] = frag<BKS, PERM>(ib, wn + 32 * t, kk, lane);
      }
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[tm], fb[tn], acc[tm][tn], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      char* na = smem + ((kt + 1) & 1) * 2 * IMG;
      store_lds<AKS>(na, va);
      store_lds<BKS>(na + IMG, vb);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- GEMM: epilogue
// v = mul (acc + add E[row][col]) for the epilogue addend E (same shape and leading dimension as C), or mul acc.
// Accumulator register 4 q + e of lane l: row 8 q + 4 h + e, column l & 31.  `mirror`: C is symmetric and this tile
// has tj >= ti: the transposed element is written from the same value (4 consecutive columns: one 8-byte store);
// a diagonal tile writes its elements on and above the diagonal, and mirrors those above it.
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[2][2], u16* __restrict__ C, const u16* __restrict__ E,
                                         int M, int N, int m0, int n0, float add, float mul, bool mirror) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const bool diag = mirror && m0 == n0;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int col = n0 + (wave & 1) * 64 + 32 * tn + (lane & 31);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = m0 + (wave >> 1) * 64 + 32 * tm + 8 * q + 4 * h;  // rows row .. row + 3; M is a multiple of 8
        if (row >= M || col >= N) continue;
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[tm][tn][4 * q + e];
          if (E != nullptr) v = fmaf(add, bf16_to_f(E[(int64_t)(row + e) * N + col]), v);
          o[e] = f_to_bf16(v * mul);
        }
        if (!diag) {
#pragma unroll
          for (int e = 0; e < 4; ++e) C[(int64_t)(row + e) * N + col] = o[e];
          if (mirror) *reinterpret_cast<u16x4*>(C + (int64_t)col * N + row) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (col >= row + e) C[(int64_t)(row + e) * N + col] = o[e];
            if (col > row + e) C[(int64_t)col * N + row + e] = o[e];
          }
        }
      }
    }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
}

// One workgroup per tile of the table.  xin: the X buffer this iteration reads.  first: the first iteration, whose
// epilogues carry the normalisation.  mirror: the table lists tj >= ti only (stages 1 and 2).
template <int STAGE>
__global__ __launch_bounds__(kBlock) void muon_stage_kernel(const Problem* __restrict__ problems,
                                                            const Tile* __restrict__ tiles, u16* __restrict__ ws,
                                                            const float* __restrict__ scale, int xin, int first,
                                                            int mirror) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Tile t = tiles[blockIdx.x];
  const Problem p = problems[t.problem];
  const int r = (int)p.rows, c = (int)p.cols;
  const bool tall = r > c;
  const int m = tall ? c : r, n = tall ? r : c;
  const int m0 = t.ti * BM, n0 = t.tj * BN;
  const float s = first ? scale[t.problem] : 1.f;
  f32x16 acc[2][2];
  zero_acc(acc);
  if constexpr (STAGE == 1) {
    const u16* X = ws + (xin ? p.x[1] : p.x[0]);
    if (tall) gemm_tile<true, true>(X, c, X, c, m, m, n, m0, n0, smem, acc);
    else gemm_tile<false, false>(X, c, X, c, m, m, n, m0, n0, smem, acc);
    epilogue(acc, ws + p.a, nullptr, m, m, m0, n0, 0.f, s * s, mirror != 0);
  } else if constexpr (STAGE == 2) {
    const u16* A = ws + p.a;
    gemm_tile<false, false>(A, m, A, m, m, m, m, m0, n0, smem, acc);
    // c (A A) is rounded to fp32 once; b A joins it inside one fma
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] *= kC;
    epilogue(acc, ws + p.b, A, m, m, m0, n0, kB, 1.f, mirror != 0);
  } else {
    const u16* X = ws + (xin ? p.x[1] : p.x[0]);
    const u16* Bm = ws + p.b;
    if (tall) gemm_tile<false, false>(X, c, Bm, m, r, c, m, m0, n0, smem, acc);
    else gemm_tile<false, true>(Bm, m, X, c, r, c, m, m0, n0, smem, acc);
    epilogue(acc, ws + (xin ? p.x[0] : p.x[1]), X, r, c, m0, n0, kA, s, false);
  }
}

// ---------------------------------------------------------------- the surrounding passes
// The block's sum in a fixed order: shuffles inside the wave, waves in wave order.  Every thread calls it.
__device__ __forceinline__ float block_sum(float v) {
  __shared__ float part[kBlock / 64];
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = part[0];
#pragma unroll
  for (int k = 1; k < kBlock / 64; ++k) t += part[k];
  __syncthreads();
  return t;
}

// Chunk ch covers flat elements [lo, hi) of problem chunk_problem[ch]; lo and hi are multiples of 4 (a Muon matrix
// has a multiple of 64 elements at a 4-aligned offset), so every access is a whole group of 4.
template <bool LP>
__global__ __launch_bounds__(kBlock) void muon_momentum_kernel(void* __restrict__ g, float* __restrict__ mom,
                                                               const int64_t* __restrict__ chunk_lo,
                                                               const int64_t* __restrict__ chunk_hi,
                                                               const int* __restrict__ chunk_problem, int n_chunks,
                                                               const Problem* __restrict__ problems,
                                                               u16* __restrict__ ws, const float* __restrict__ hp,
                                                               const float* __restrict__ state,
                                                               float* __restrict__ partials) {
#pragma clang fp contract(off)
  const bool skip = state != nullptr && state[3] != 0.f;
  const float gscale = state != nullptr ? state[1] : 1.f;
  const float mu = hp[7];
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t lo = chunk_lo[ch], hi = chunk_hi[ch];
    const Problem p = problems[chunk_problem[ch]];
    u16* __restrict__ u = ws + p.x[0] - p.flat;  // indexed by the flat element
    float ss = 0.f;
    for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * kBlock) {
      float gv[4];
      if constexpr (LP) {
        u16* gp = static_cast<u16*>(g) + i;
        const u16x4 t = *reinterpret_cast<const u16x4*>(gp);
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = bf16_to_f(t[e]);
        *reinterpret_cast<u16x4*>(gp) = u16x4{0, 0, 0, 0};
      } else {
        float* gp = static_cast<float*>(g) + i;
        const f32x4 t = *reinterpret_cast<const f32x4*>(gp);
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = t[e];
        *reinterpret_cast<f32x4*>(gp) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      if (skip) continue;
      f32x4 mv = *reinterpret_cast<const f32x4*>(mom + i);
      u16x4 ub;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ge = gv[e] * gscale;
        mv[e] = fmaf(mu, mv[e], ge);
        ub[e] = f_to_bf16(fmaf(mu, mv[e], ge));
        const float ur = bf16_to_f(ub[e]);
        ss = fmaf(ur, ur, ss);
      }
      *reinterpret_cast<f32x4*>(mom + i) = mv;
      *reinterpret_cast<u16x4*>(u + i) = ub;
    }
    const float total = block_sum(ss);
    if (threadIdx.x == 0 && !skip) partials[ch] = total;
  }
}

__global__ __launch_bounds__(64) void muon_norm_kernel(const float* __restrict__ partials,
                                                       const int* __restrict__ first, const int* __restrict__ count,
                                                       float* __restrict__ scale) {
  const int p = blockIdx.x;
  const int f = first[p], n = count[p];
  double a = 0.0;
  for (int k = threadIdx.x; k < n; k += 64) a += (double)partials[f + k];
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if (threadIdx.x == 0) scale[p] = 1.f / ((float)sqrt(a) + 1e-7f);
}

template <bool LP>
__global__ __launch_bounds__(kBlock) void muon_update_kernel(float* __restrict__ w, u16* __restrict__ wlp,
                                                             const int64_t* __restrict__ chunk_lo,
                                                             const int64_t* __restrict__ chunk_hi,
                                                             const int* __restrict__ chunk_problem, int n_chunks,
                                                             const Problem* __restrict__ problems,
                                                             const u16* __restrict__ ws, int xout,
                                                             const float* __restrict__ hp,
                                                             const float* __restrict__ sched,
                                                             const float* __restrict__ state) {
#pragma clang fp contract(off)
  if (state != nullptr && state[3] != 0.f) return;
  float lr = hp[6];
  if (sched != nullptr && sched[0] > 0.f) lr *= hp[0] / sched[0];
  const float keep = 1.f - lr * hp[4];
  for (int ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const int64_t lo = chunk_lo[ch], hi = chunk_hi[ch];
    const Problem p = problems[chunk_problem[ch]];
    const u16* __restrict__ o = ws + (xout ? p.x[1] : p.x[0]) - p.flat;
    const float ratio = (float)p.rows / (float)p.cols;
    const float step = lr * sqrtf(ratio > 1.f ? ratio : 1.f);
    for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * kBlock) {
      f32x4 wv = *reinterpret_cast<const f32x4*>(w + i);
      const u16x4 ov = *reinterpret_cast<const u16x4*>(o + i);
      u16x4 lp;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        wv[e] = fmaf(-step, bf16_to_f(ov[e]), wv[e] * keep);
        lp[e] = f_to_bf16(wv[e]);
      }
      *reinterpret_cast<f32x4*>(w + i) = wv;
      if constexpr (LP) *reinterpret_cast<u16x4*>(wlp + i) = lp;
    }
  }
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline int grid_for(int n) { return n < kGridCap ? n : kGridCap; }

template <int STAGE>
int launch_stage(const Problem* problems, const Tile* tiles, int n_tiles, u16* ws, const float* scale, int xin,
                 int first, int mirror, hipStream_t stream) {
  hipLaunchKernelGGL(muon_stage_kernel<STAGE>, dim3(n_tiles), dim3(kBlock), kSmem, stream, problems, tiles, ws, scale,
                     xin, first, mirror);
  return (int)hipGetLastError();
}

}  // namespace

PLX_API int plx_muon_chunk() { return kChunk; }
PLX_API int plx_muon_tile() { return BM; }
PLX_API int plx_muon_problem_size() { return (int)sizeof(Problem); }

// Set the kernels' LDS attribute ahead of a stream capture (hipFuncSetAttribute is not a stream operation).
PLX_API int plx_muon_prepare() {
  static bool ready = false;
  if (ready) return 0;
  ready = true;
  return hipFuncSetAttribute((const void*)muon_stage_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem) ||
                 hipFuncSetAttribute((const void*)muon_stage_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSmem) ||
                 hipFuncSetAttribute((const void*)muon_stage_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSmem)
             ? 3
             : 0;
}

// lp: g is bf16 (indexed by the flat element, like mom), else fp32.  partials holds n_chunks floats.
PLX_API int plx_muon_momentum(int lp, void* g, float* mom, const int64_t* chunk_lo, const int64_t* chunk_hi,
                              const int* chunk_problem, int n_chunks, const void* problems, void* ws,
                              const float* hp, const float* state, float* partials, hipStream_t stream) {
  if (n_chunks == 0) return 0;
  if (n_chunks < 0 || !g || !mom || !chunk_lo || !chunk_hi || !chunk_problem || !problems || !ws || !hp || !partials)
    return 1;
  if ((uintptr_t)g % (lp ? 8 : 16) != 0 || !aligned16(mom) || !aligned16(ws)) return 1;
  const Problem* pr = static_cast<const Problem*>(problems);
  const dim3 grid(grid_for(n_chunks)), block(kBlock);
  if (lp)
    hipLaunchKernelGGL(muon_momentum_kernel<true>, grid, block, 0, stream, g, mom, chunk_lo, chunk_hi, chunk_problem,
                       n_chunks, pr, static_cast<u16*>(ws), hp, state, partials);
  else
    hipLaunchKernelGGL(muon_momentum_kernel<false>, grid, block, 0, stream, g, mom, chunk_lo, chunk_hi, chunk_problem,
                       n_chunks, pr, static_cast<u16*>(ws), hp, state, partials);
  return (int)hipGetLastError();
}

// scale[p] = 1 / (sqrt(sum of the partials of chunks [first[p], first[p] + count[p])) + 1e-7)
PLX_API int plx_muon_norms(const float* partials, const int* first, const int* count, int n_problems, float* scale,
                           hipStream_t stream) {
  if (n_problems == 0) return 0;
  if (n_problems < 0 || !partials || !first || !count || !scale) return 1;
  hipLaunchKernelGGL(muon_norm_kernel, dim3(n_problems), dim3(64), 0, stream, partials, first, count, scale);
  return (int)hipGetLastError();
}

// One stage (1, 2 or 3) of one iteration over a tile table.  tiles: n_tiles x int4 (problem, tile row, tile column,
// 0) in 128 x 128 tiles of the stage's output: m x m (stages 1, 2) or rows x cols (stage 3).  mirror (stages 1, 2):
// the table lists only tile column >= tile row.  xin: the X buffer read (stage 3 writes the other one).
PLX_API int plx_muon_stage(int stage, int first_iteration, const void* problems, const void* tiles, int n_tiles,
                           void* ws, const float* scale, int xin, int mirror, hipStream_t stream) {
  if (n_tiles == 0) return 0;
  if (n_tiles < 0 || !problems || !tiles || !ws || !aligned16(ws) || (xin != 0 && xin != 1)) return 1;
  if (first_iteration && !scale) return 1;
  if (plx_muon_prepare() != 0) return 3;  // the LDS images need more than the default 64 KiB
  const Problem* pr = static_cast<const Problem*>(problems);
  const Tile* tl = static_cast<const Tile*>(tiles);
  u16* w = static_cast<u16*>(ws);
  if (stage == 1) return launch_stage<1>(pr, tl, n_tiles, w, scale, xin, first_iteration, mirror, stream);
  if (stage == 2) return launch_stage<2>(pr, tl, n_tiles, w, scale, xin, first_iteration, mirror, stream);
  if (stage == 3) return launch_stage<3>(pr, tl, n_tiles, w, scale, xin, first_iteration, 0, stream);
  return 1;
}

// w (fp32 master, and wlp, the bf16 model copy, when given) over the chunks; xout: the X buffer holding O.
PLX_API int plx_muon_update(float* w, void* wlp, const int64_t* chunk_lo, const int64_t* chunk_hi,
                            const int* chunk_problem, int n_chunks, const void* problems, const void* ws, int xout,
                            const float* hp, const float* sched, const float* state, hipStream_t stream) {
  if (n_chunks == 0) return 0;
  if (n_chunks < 0 || !w || !chunk_lo || !chunk_hi || !chunk_problem || !problems || !ws || !hp) return 1;
  if (!aligned16(w) || (uintptr_t)wlp % 8 != 0 || !aligned16(ws) || (xout != 0 && xout != 1)) return 1;
  const Problem* pr = static_cast<const Problem*>(problems);
  const dim3 grid(grid_for(n_chunks)), block(kBlock);
  if (wlp)
    hipLaunchKernelGGL(muon_update_kernel<true>, grid, block, 0, stream, w, static_cast<u16*>(wlp), chunk_lo,
                       chunk_hi, chunk_problem, n_chunks, pr, static_cast<const u16*>(ws), xout, hp, sched, state);
  else
    hipLaunchKernelGGL(muon_update_kernel<false>, grid, block, 0, stream, w, static_cast<u16*>(nullptr), chunk_lo,
                       chunk_hi, chunk_problem, n_chunks, pr, static_cast<const u16*>(ws), xout, hp, sched, state);
  return (int)hipGetLastError();
}
