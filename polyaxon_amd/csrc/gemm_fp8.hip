// FP8 GEMM for the language-model linears on MI355X (gfx950), with per-tensor power-of-two scales kept on the device:
// gemm_edge.hip's structure on byte operands and the 128-deep f8f6f4 MFMA.
//
//   plx_fp8_amax   amax = max |x| of a bf16 tensor, scale = 2^floor(log2(FMAX / amax)) (1 when amax is 0 or not finite)
//                  and 1 / scale, three fp32 device words.  FMAX = 448 (E4M3) or 57344 (E5M2).
//   plx_fp8_cast   bf16 [R][C] -> FP8 [R][C] and FP8 [C][R] in one read: x * scale, clamped to +-FMAX, v_cvt_pk_*_f32.
//   plx_gemm_fp8   C[M][N] = (ia * ib * alpha) * sum_k A[m][k] B[n][k]  (+ C) (+ bias[n]) (second store: gelu_tanh),
//                  C bf16 (ldc), A (E4M3 or E5M2) and B (E4M3) both K-MAJOR bytes, ia / ib POINTERS to the operands'
//                  inverse scales (read in the epilogue: no host sync, capturable).  M, N, K multiples of 16.
//
// The GEMM:
//   * Tile 128 x 128 x 128, 256 threads = 4 waves as 2 (M) x 2 (N), two blocks per CU; each wave owns 64 x 64 of C as
//     4 x 4 tiles of v_mfma_f32_16x16x128_f8f6f4 (64 accumulator registers, 16 MFMAs per K-tile).  The MFMA's A
//     operand is B's rows (n, always E4M3: cbsz = 0) and its B operand A's rows (m, the format in blgp), so a lane's
//     accumulator holds 4 consecutive n of one m: 8-byte bf16 stores.  The 16x16x128 form keeps gemm_edge's
//     accumulator layout and epilogue; the 32x32x64 form was not tried.
//   * LDS: 2 stages x (A 16 KiB + B 16 KiB) = 64 KiB.  A K-tile row is 128 B as in gemm_edge.hip, so the operand
//     image is the same: 128 rows of 128 B, physical 16-byte chunk = logical ^ kswz(row), staged by buffer-resource
//     LDS-DMA in sixteen 1 KiB pieces (four per wave) with the swizzle applied to the per-lane SOURCE chunk.
//   * Fragments: lane (fr = lane & 15, fq = lane >> 4) holds row c0 + fr, bytes 32 fq .. 32 fq + 31 of the K-tile:
//     logical chunks 2 fq and 2 fq + 1, two ds_read_b128.  A and B use the same addressing, so whichever k each
//     register byte holds, the two operands agree.
//   * Bank conflicts.  A ds_read_b128 is served 16 lanes at a time, and the 16 lanes of one fq read one logical
//     chunk c (2 fq, then 2 fq + 1) of rows 0..15 of a 16-row tile.  Rows 2 j and 2 j + 1 share kswz = j and lie in
//     the two 128-byte halves of one 256-byte line of the 64 banks; over j = 0..7 the physical chunk c ^ j takes all
//     8 values.  So the 16 lanes touch 8 chunks x 2 halves = 16 different 16-byte bank groups: each of the 64 banks
//     once, for every c -- the argument of gemm_edge.hip, which holds for any fixed logical chunk and so for both
//     reads of a fragment.
//   * One barrier per K-tile (wait for this wave's DMAs of tile t, barrier, read t's fragments, issue t + 1's DMAs
//     into the other stage, 16 MFMAs); the CU's second block covers the barrier.
//   * Tails cost no branch in the K loop: an operand's resource ends at its true last byte, so rows past the end read
//     zeros, and a chunk at k >= K (the last K-tile only) selects an out-of-range offset.  Both operands are masked.
//   * Epilogue: v = acc * (ia * ib * alpha), then + C or + bias, masked 8-byte stores; with the GELU flag the stored
//     bf16 value's gelu_tanh (gemm256.hip's formula) goes to a second buffer laid out like C.
//   * Split-K when the tile grid cannot fill the chip (weight gradients, K = tokens): blockIdx.y owns whole K-tiles,
//     the last split is ragged, each split stores an fp32 slab of raw sums and gemm_fp8_reduce adds them in split
//     order, then applies the scales and the epilogue.  No atomics: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLX_API extern "C" __attribute__((visibility("default")))

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int E4M3 = 0, E5M2 = 1;  // also the MFMA's format codes (cbsz / blgp)
__host__ __device__ constexpr float fmax_of(int fmt) { return fmt == E5M2 ? 57344.f : 448.f; }

// ------------------------------------------------------------------------------------------------ amax and scale
constexpr int AMAX_MAX_BLOCKS = 1024;

// state: two zeroed uint32 words (running max of the |x| bit patterns, arrival ticket), left zeroed again.
// words: fp32 [amax, scale, 1 / scale].  |x| bit patterns order like the values (NaN above inf), so the unsigned
// integer max is the float max whatever the order of arrival.
__global__ void __launch_bounds__(256) fp8_amax_kernel(const uint4* __restrict__ x, long long n8, unsigned* state,
                                                       float* __restrict__ words, float fmax) {
  __shared__ unsigned sh[4];
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const uint4 v = x[i];  // 8 bf16: |x| as fp32 bits is the half word shifted up
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m = max(m, (w[j] << 16) & 0x7fffffffu);
      m = max(m, w[j] & 0x7fff0000u);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  m = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
  // both atomics execute at the L2; the ticket is taken only after the max has returned
  const unsigned before = __hip_atomic_fetch_max(state, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(before) : "memory");
  const unsigned ticket = __hip_atomic_fetch_add(state + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != gridDim.x - 1) return;
  const unsigned bits = __hip_atomic_exchange(state, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(state + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float amax = __uint_as_float(bits);
  float scale = 1.f;
  if (bits != 0 && bits < 0x7f800000u) {
    const float q = fmax / amax;  // IEEE division; its exponent is floor(log2 q)
    const int e = min((int)(__float_as_uint(q) >> 23) - 127, 126);  // <= 126: 1 / scale stays normal
    scale = __uint_as_float((unsigned)(e + 127) << 23);
  }
  words[0] = amax;
  words[1] = scale;
  words[2] = 1.f / scale;
}

// ------------------------------------------------------------------------------------------------ cast + transpose
template <int FMT>
__device__ __forceinline__ unsigned cvt4(float a, float b, float c, float d) {
  int w = 0;
  if (FMT == E5M2) {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  }
  return (unsigned)w;
}

// A block converts a 64 x 64 tile.  Pass p: thread (r = 32 p + tid / 8, c8 = tid & 7) loads 8 bf16 (16 B), stores
// their 8 FP8 bytes row-major and into the LDS tile: 64 rows of 64 B, physical 8-byte chunk = c8 ^ (r >> 3).  Any 32
// lanes of the ds_write_b64 cover 4 whole rows = 256 contiguous bytes, whatever the permutation inside a row.
// Transposed pass i: thread (c = 32 i + tid / 8, g = tid & 7) gathers input column c of rows 8 g .. 8 g + 7 with 8
// ds_read_b32 (a wave's 8 columns lie in one 8-byte chunk): at step j the 8 row groups read rows 8 g + j, which share
// the 64-byte quarter (row & 3) of the banks and differ in their swizzle g, so they hit 8 different chunks; lanes of
// one g that share a word are a broadcast.  Both directions store 8 bytes per lane, 64 contiguous bytes per 8 lanes.
template <int FMT>
__global__ void __launch_bounds__(256) fp8_cast_kernel(const __bf16* __restrict__ x, uint8_t* __restrict__ q,
                                                       uint8_t* __restrict__ qt, int R, int C,
                                                       const float* __restrict__ words) {
  __shared__ __attribute__((aligned(16))) unsigned tile[64 * 16];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float s = words[1], lim = fmax_of(FMT);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int rl = 32 * p + (tid >> 3), c8 = tid & 7;
    const int r = r0 + rl, c = c0 + 8 * c8;
    if (r < R && c < C) {  // C is a multiple of 8: the chunk is inside or outside as a whole
      const uint4 v = *(const uint4*)(x + (size_t)r * C + c);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      float f[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[2 * j] = fminf(fmaxf(__uint_as_float(w[j] << 16) * s, -lim), lim);
        f[2 * j + 1] = fminf(fmaxf(__uint_as_float(w[j] & 0xffff0000u) * s, -lim), lim);
      }
      const uint2 o = make_uint2(cvt4<FMT>(f[0], f[1], f[2], f[3]), cvt4<FMT>(f[4], f[5], f[6], f[7]));
      *(uint2*)(q + (size_t)r * C + c) = o;
      *(uint2*)(tile + rl * 16 + 2 * (c8 ^ (rl >> 3))) = o;
    }
  }
  __syncthreads();
  const int g = tid & 7;  // row group: rows 8 g .. 8 g + 7
  if (r0 + 8 * g >= R) return;  // R is a multiple of 8
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cl = 32 * i + (tid >> 3);
    if (c0 + cl >= C) continue;
    const int sh = 8 * (cl & 3), wcol = (cl >> 2) & 1, ch = cl >> 3;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rl = 8 * g + j;
      const unsigned b = (tile[rl * 16 + 2 * (ch ^ g) + wcol] >> sh) & 0xffu;
      if (j < 4) lo |= b << (8 * j);
      else hi |= b << (8 * (j - 4));
    }
    *(uint2*)(qt + (size_t)(c0 + cl) * R + r0 + 8 * g) = make_uint2(lo, hi);
  }
}

// ------------------------------------------------------------------------------------------------ the GEMM
constexpr int BM = 128, BN = 128, BK = 128, NTH = 256, NW = 4;
constexpr int IMG = 16384;            // one operand's K-tile: 128 rows x 128 B
constexpr int STAGE = 2 * IMG;        // [A | B]
constexpr int LDS_BYTES = 2 * STAGE;  // 64 KiB: two blocks per CU
constexpr int PIECES = IMG / 1024 / NW;  // 1 KiB DMA pieces per wave per image

// An offset no resource of this file contains: every extent is at most 2^31 bytes.
constexpr uint32_t OOB = 0x80000000u;

// physical 16-B chunk = logical ^ kswz(row)
__device__ __forceinline__ int kswz(int row) { return (row >> 1) & 7; }

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

// ids walk `group` M-tiles of one N-column, then the next column (consecutive ids share an XCD and its L2)
__device__ __forceinline__ void tile_of(int id, int ntm, int ntn, int group, int& tm, int& tn) {
  const int per = group * ntn;
  const int first = (id / per) * group;
  const int gs = min(ntm - first, group);
  const int r = id - (id / per) * per;
  tm = first + r % gs;
  tn = r / gs;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// the whole offset travels in the VGPR, which is what the range check sees
__device__ __forceinline__ void glds(__amdgpu_buffer_rsrc_t r, uint32_t off, void* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)l, 16, off, 0, 0, 0);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)b) << 16);
}

__device__ __forceinline__ float bf16_round(float f) { return (float)(__bf16)f; }

// gemm256.hip's GELU (tanh approximation) of the bf16-rounded value
__device__ __forceinline__ float gelu_tanh(float h) {
  const float u = 0.7978845608028654f * fmaf(0.044715f * h * h, h, h);
  return 0.5f * h * (2.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * u)));
}

template <int V>
struct IC {
  static constexpr int value = V;
};

struct Fp8Args {
  const uint8_t* A;   // [M][lda] bytes, K-major
  const uint8_t* B;   // [N][ldb] bytes, K-major, E4M3
  void* C;            // bf16 [M][ldc], or fp32 slabs [splits][M][N] when K is split
  void* C2;           // bf16 [M][ldc]: gelu_tanh of the stored C, or null
  int M, N, K, lda, ldb, ldc;
  int kt_per_split;   // K-tiles per blockIdx.y
  float alpha;
  const float* ia;    // the operands' inverse scales (one fp32 device word each)
  const float* ib;
  const float* bias;  // fp32 [N] or null
  int group;          // M-tiles per tile group (tile_of)
};

// One operand's staging: the resource, and per DMA piece of this wave the lane's source offset at K-tile 0 with its
// swizzled chunk folded in.  R rows of which the tile starts at r0; the block's K range starts at kbeg.
struct Stager {
  __amdgpu_buffer_rsrc_t r;
  uint32_t off[PIECES];
  int klim[PIECES];  // the chunk is inside its row while 128 kt < klim

  __device__ __forceinline__ Stager(const uint8_t* X, int ld, int R, int K, int r0, int kbeg, int wave, int lane) {
    // bytes from the tile origin to the operand's true last byte + 1 (a multiple of 16; r0 < R, kbeg < K)
    const size_t bytes = (size_t)(R - 1 - r0) * ld + (K - kbeg);
    r = rsrc(X + (size_t)r0 * ld + kbeg, bytes < OOB ? (uint32_t)bytes : OOB);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int row = (wave + NW * i) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ kswz(row);
      off[i] = (uint32_t)(row * ld + chunk * 16);
      klim[i] = K - kbeg - chunk * 16;
    }
  }

  // DMA this wave's pieces of K-tile kt (relative to kbeg) into the image at `img`
  __device__ __forceinline__ void issue(int kt, char* img, int wave) const {
#pragma unroll
    for (int i = 0; i < PIECES; ++i)
      glds(r, kt * BK < klim[i] ? off[i] + (uint32_t)(kt * BK) : OOB, img + (wave + NW * i) * 1024);
  }
};

__device__ __forceinline__ i32x8 ld_frag(const char* img, int o0, int o1) {
  const i32x4 lo = *(const i32x4*)(img + o0), hi = *(const i32x4*)(img + o1);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// acc += the wave's 64 x 64 part of the tile at (m0, n0) over K-tiles [kt0, kt0 + nk)
template <int AFMT>
__device__ __forceinline__ void fp8_tile(const Fp8Args& p, int m0, int n0, int kt0, int nk, f32x4 (&acc)[4][4],
                                         char* smem, int wave, int lane, int wm, int wn) {
  const Stager sa(p.A, p.lda, p.M, p.K, m0, kt0 * BK, wave, lane);
  const Stager sb(p.B, p.ldb, p.N, p.K, n0, kt0 * BK, wave, lane);

  // kswz(c0 + fr) = kswz(fr) for a 16-aligned c0: the two chunk offsets depend on the lane only; tile t adds 2048 B
  const int fr = lane & 15, fq = lane >> 4;
  const int o0 = fr * 128 + (((2 * fq) ^ kswz(fr)) << 4), o1 = fr * 128 + (((2 * fq + 1) ^ kswz(fr)) << 4);
  const int abase = wm * 64 * 128, bbase = wn * 64 * 128;

  auto step = [&](auto cb, int kt) {
    constexpr int CB = decltype(cb)::value;
    const char* ia = smem + CB * STAGE + abase;
    const char* ib = smem + CB * STAGE + IMG + bbase;
    // this wave's DMAs of tile kt have landed and its earlier LDS reads are done; after the barrier, everyone's
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    i32x8 fa[4], fb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fa[t] = ld_frag(ia + t * 2048, o0, o1);
      fb[t] = ld_frag(ib + t * 2048, o0, o1);
    }
    if (kt + 1 < nk) {  // the other stage: last read in step kt - 1, before the barrier above
      sa.issue(kt + 1, smem + (1 - CB) * STAGE, wave);
      sb.issue(kt + 1, smem + (1 - CB) * STAGE + IMG, wave);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)  // zero scale operands: the unscaled instruction
        acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[nt], fa[mt], acc[nt][mt], E4M3, AFMT, 0, 0,
                                                                       0, 0);
  };

  sa.issue(0, smem, wave);
  sb.issue(0, smem + IMG, wave);
  for (int kt = 0; kt < nk; kt += 2) {
    step(IC<0>{}, kt);
    if (kt + 1 < nk) step(IC<1>{}, kt + 1);
  }
}

// ACC: C += s * AB (bf16 read-modify-write); SLAB: write fp32 raw sums (split K)
template <int AFMT, bool ACC, bool SLAB>
__global__ void __launch_bounds__(NTH, 2) gemm_fp8_kernel(Fp8Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  int tm, tn;
  tile_of(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, p.group, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt0 = blockIdx.y * p.kt_per_split;
  const int nk = min(p.kt_per_split, (p.K + BK - 1) / BK - kt0);

  f32x4 acc[4][4];  // [n tile][m tile] of the wave's 64 x 64
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  fp8_tile<AFMT>(p, m0, n0, kt0, nk, acc, smem, wave, lane, wm, wn);

  // acc[nt][mt] is a 16 x 16 tile D[n][m]: m = lane & 15, n = 4 (lane >> 4) + j, j = 0..3
  const float s = SLAB ? 1.f : p.ia[0] * p.ib[0] * p.alpha;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = n0 + wn * 64 + nt * 16 + 4 * fq;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f};
    if (!SLAB && !ACC && p.bias != nullptr && n < p.N) bias = *(const f32x4*)(p.bias + n);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = m0 + wm * 64 + mt * 16 + fr;
      if (m >= p.M || n >= p.N) continue;
      f32x4 v = acc[nt][mt];
      if (SLAB) {
        *(f32x4*)((float*)p.C + ((size_t)blockIdx.y * p.M + m) * p.N + n) = v;
        continue;
      }
      __bf16* dst = (__bf16*)p.C + (size_t)m * p.ldc + n;
      if (ACC) {
        const uint2 o = *(const uint2*)dst;
        v[0] = s * v[0] + __uint_as_float(o.x << 16);
        v[1] = s * v[1] + __uint_as_float(o.x & 0xffff0000u);
        v[2] = s * v[2] + __uint_as_float(o.y << 16);
        v[3] = s * v[3] + __uint_as_float(o.y & 0xffff0000u);
      } else {
        v = v * s + bias;
      }
      *(uint2*)dst = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
      if (!ACC && p.C2 != nullptr)
        *(uint2*)((__bf16*)p.C2 + (size_t)m * p.ldc + n) =
            make_uint2(pack_bf16x2(gelu_tanh(bf16_round(v[0])), gelu_tanh(bf16_round(v[1]))),
                       pack_bf16x2(gelu_tanh(bf16_round(v[2])), gelu_tanh(bf16_round(v[3]))));
    }
  }
}

// C (bf16, ldc) = ia ib alpha * sum over splits (in split order) of the fp32 slabs (+ bias) (+ C when accumulating)
// (C2: gelu_tanh of the stored C); 8 elements per thread (N is a multiple of 8: a thread's 8 stay in one row)
template <bool ACC>
__global__ void __launch_bounds__(256) gemm_fp8_reduce(const float* __restrict__ ws, __bf16* __restrict__ C,
                                                       __bf16* __restrict__ C2, int M, int N, int ldc, int splits,
                                                       float alpha, const float* __restrict__ ia,
                                                       const float* __restrict__ ib, const float* __restrict__ bias) {
  const size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i8 >= (size_t)M * N / 8) return;
  const size_t e = i8 * 8;
  const int m = (int)(e / N), n = (int)(e % N);
  f32x4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const size_t slab = (size_t)M * N;
  for (int k = 0; k < splits; ++k) {
    const f32x4* src = (const f32x4*)(ws + k * slab + e);
    s[0] += src[0];
    s[1] += src[1];
  }
  const float sc = ia[0] * ib[0] * alpha;
  s[0] *= sc;
  s[1] *= sc;
  if (bias != nullptr) {
    s[0] += *(const f32x4*)(bias + n);
    s[1] += *(const f32x4*)(bias + n + 4);
  }
  __bf16* dst = C + (size_t)m * ldc + n;
  if (ACC) {
    const uint4 o = *(const uint4*)dst;
    const unsigned w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j >> 1][2 * (j & 1)] += __uint_as_float(w[j] << 16);
      s[j >> 1][2 * (j & 1) + 1] += __uint_as_float(w[j] & 0xffff0000u);
    }
  }
  *(uint4*)dst = make_uint4(pack_bf16x2(s[0][0], s[0][1]), pack_bf16x2(s[0][2], s[0][3]), pack_bf16x2(s[1][0], s[1][1]),
                            pack_bf16x2(s[1][2], s[1][3]));
  if (!ACC && C2 != nullptr) {
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = gelu_tanh(bf16_round(s[j >> 2][j & 3]));
    *(uint4*)(C2 + (size_t)m * ldc + n) =
        make_uint4(pack_bf16x2(g[0], g[1]), pack_bf16x2(g[2], g[3]), pack_bf16x2(g[4], g[5]), pack_bf16x2(g[6], g[7]));
  }
}

template <int AFMT, bool ACC, bool SLAB>
int launch(const Fp8Args& a, int splits, hipStream_t st) {
  auto k = gemm_fp8_kernel<AFMT, ACC, SLAB>;
  static const int attr =
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess ? 0 : -4;
  if (attr) return attr;
  const dim3 grid(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), splits);
  hipLaunchKernelGGL(k, grid, dim3(NTH), LDS_BYTES, st, a);
  return 0;
}

template <int AFMT>
int dispatch(const Fp8Args& a, int splits, int accumulate, hipStream_t st) {
  if (splits > 1) return launch<AFMT, false, true>(a, splits, st);
  return accumulate ? launch<AFMT, true, false>(a, 1, st) : launch<AFMT, false, false>(a, 1, st);
}

constexpr int kSplitTarget = 512;  // blocks the split-K planner aims for: two per CU of a 256-CU chip
constexpr int kGroup = 4;

bool shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 16 == 0 && N % 16 == 0 && K % 16 == 0; }

// K-tiles per split: the most blocks (tiles x splits) up to kSplitTarget with every split but the last >= 8 K-tiles.
// A pure function of the shape (the same plan on every rank and every run).
int plan_kt_per_split(int M, int N, int K) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN), nk = (K + BK - 1) / BK;
  int best = nk, best_blocks = tiles;
  for (int s = 2; 2 * tiles <= kSplitTarget && s <= nk / 8; ++s) {
    const int kps = (nk + s - 1) / s;
    if (kps < 8) break;
    const int blocks = tiles * ((nk + kps - 1) / kps);
    if (blocks > kSplitTarget) break;
    if (blocks > best_blocks) best = kps, best_blocks = blocks;
  }
  return best;
}

}  // namespace

// number of K splits (blockIdx.y) for this shape: 1 = no workspace needed, 0 = a shape the kernel does not take
PLX_API int plx_gemm_fp8_splits(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return 0;
  const int kps = plan_kt_per_split(M, N, K);
  return ((K + BK - 1) / BK + kps - 1) / kps;
}

// fp32 workspace floats the launch needs (0 when K is not split, -1 for a shape the kernel does not take)
PLX_API long long plx_gemm_fp8_ws(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return -1;
  const int s = plx_gemm_fp8_splits(M, N, K);
  return s > 1 ? (long long)s * M * N : 0;
}

PLX_API int plx_gemm_fp8_tile() { return BM; }

// blocks of the amax launch for n elements
PLX_API int plx_fp8_amax_blocks(long long n) {
  const long long b = (n / 8 + 2047) / 2048;  // >= 8 chunks per thread before a second block is worth its ticket
  return (int)(b < 1 ? 1 : b > AMAX_MAX_BLOCKS ? AMAX_MAX_BLOCKS : b);
}

// words[0..2] = amax, scale, 1 / scale of the bf16 tensor x (n elements, n % 8 == 0, 16-byte aligned) for format
// fmt (0 = E4M3, 1 = E5M2).  state: two zeroed uint32 words of this stream, zero again when the kernel ends.
PLX_API int plx_fp8_amax(const void* x, long long n, int fmt, void* state, float* words, void* stream) {
  if (n <= 0 || n % 8 || (uintptr_t)x % 16 || (fmt != E4M3 && fmt != E5M2) || !state || !words) return -1;
  hipLaunchKernelGGL(fp8_amax_kernel, dim3(plx_fp8_amax_blocks(n)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x,
                     n / 8, (unsigned*)state, words, fmax_of(fmt));
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// q [R][C] and qt [C][R] (FP8 bytes of format fmt) = x [R][C] (bf16) * words[1], clamped; R, C multiples of 16
PLX_API int plx_fp8_cast(const void* x, void* q, void* qt, int R, int C, int fmt, const float* words, void* stream) {
  if (R <= 0 || C <= 0 || R % 16 || C % 16 || (fmt != E4M3 && fmt != E5M2)) return -1;
  if ((uintptr_t)x % 16 || (uintptr_t)q % 8 || (uintptr_t)qt % 8 || !words) return -1;
  const dim3 grid((C + 63) / 64, (R + 63) / 64);
  if (grid.y > 65535) return -2;
  if (fmt == E5M2)
    hipLaunchKernelGGL(fp8_cast_kernel<E5M2>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, (uint8_t*)q,
                       (uint8_t*)qt, R, C, words);
  else
    hipLaunchKernelGGL(fp8_cast_kernel<E4M3>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, (uint8_t*)q,
                       (uint8_t*)qt, R, C, words);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// C[M][N] (bf16, ldc) = ia[0] * ib[0] * alpha * A . B^T (+ bias[n]) (+ C when accumulate); A [M][lda] bytes of format
// a_fmt, B [N][ldb] E4M3 bytes; M, N, K multiples of 16.  bias: fp32 [N], 16-byte aligned, or null (not combined with
// accumulate).  gelu_out: bf16 laid out like C receiving gelu_tanh(C), or null (not with accumulate).
// ws: plx_gemm_fp8_ws(M, N, K) floats, 16-byte aligned (may be null when that is 0).
// Returns 0, or < 0 on a shape / layout the kernel does not take (nothing launched).
PLX_API int plx_gemm_fp8(const void* A, const void* B, void* C, void* ws, int M, int N, int K, int lda, int ldb, int ldc,
                         int a_fmt, const float* ia, const float* ib, float alpha, int accumulate, const float* bias,
                         void* gelu_out, void* stream) {
  if (!shape_ok(M, N, K) || (a_fmt != E4M3 && a_fmt != E5M2) || !ia || !ib) return -1;
  if (bias != nullptr && (accumulate || (uintptr_t)bias % 16)) return -1;
  if (gelu_out != nullptr && (accumulate || (uintptr_t)gelu_out % 16)) return -1;
  if (lda % 16 || ldb % 16 || ldc % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)C % 16) return -1;
  if (lda < K || ldb < K || ldc < N) return -1;
  // the largest byte offset a block forms relative to its tile origin, tails included (it must stay below 2^31)
  if ((long long)BM * lda + K + BK >= 0x7ffffff0LL || (long long)BN * ldb + K + BK >= 0x7ffffff0LL) return -2;
  const int kps = plan_kt_per_split(M, N, K);
  const int splits = ((K + BK - 1) / BK + kps - 1) / kps;
  if (splits > 1 && (!ws || (uintptr_t)ws % 16)) return -5;
  Fp8Args a{(const uint8_t*)A, (const uint8_t*)B, splits > 1 ? ws : C, splits > 1 ? nullptr : gelu_out, M, N, K, lda,
            ldb, ldc, kps, alpha, ia, ib, bias, kGroup};
  hipStream_t st = (hipStream_t)stream;
  const int rc = a_fmt == E5M2 ? dispatch<E5M2>(a, splits, accumulate, st) : dispatch<E4M3>(a, splits, accumulate, st);
  if (rc) return rc;
  if (splits > 1) {
    const size_t total8 = (size_t)M * N / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256));
    if (accumulate)
      hipLaunchKernelGGL(gemm_fp8_reduce<true>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C, (__bf16*)nullptr, M,
                         N, ldc, splits, alpha, ia, ib, (const float*)nullptr);
    else
      hipLaunchKernelGGL(gemm_fp8_reduce<false>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C, (__bf16*)gelu_out,
                         M, N, ldc, splits, alpha, ia, ib, bias);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
