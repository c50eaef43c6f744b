// Edge-tile bf16 GEMM for the language-model linears on MI355X (gfx950): the contract of gemm256.hip for shapes that
// are not multiples of its 256 x 256 x 64 tile.
//
//   C[M][N] = alpha * sum_k A(m, k) B(n, k)   (+ C when accumulating) (+ bias[n]), C bf16 row-major (ldc)
//
// with each operand either K-MAJOR (X[r][k], k contiguous) or MN-MAJOR (X[k][r], r contiguous), fp32 accumulation, for
// every M, N, K > 0 that are multiples of 8: a 16-byte chunk of either layout is then wholly inside or wholly outside
// its matrix, rows are 16-byte aligned and the epilogue's 8-byte stores are whole.
//
//   * Tile 128 x 128 x 64, 256 threads = 4 waves as 2 (M) x 2 (N); each wave owns 64 x 64 of C as 4 x 4 tiles of
//     v_mfma_f32_16x16x32_bf16 (64 accumulator registers).  As in gemm256 the MFMA A operand is B's rows (n) and its B
//     operand A's rows (m), so a lane's accumulator holds 4 consecutive n of one m: 8-byte stores.
//   * LDS: 2 stages x (A 16 KiB + B 16 KiB) = 64 KiB, two blocks per CU.  An operand image is gemm256's "quarter":
//     K-major 128 rows of 128 B (XOR-swizzled 16-byte chunks, ds_read_b128), MN-major 64 k-rows of 256 B
//     (ds_read_b64_tr_b16, the hardware transpose).  Staging is buffer-resource LDS-DMA, 16 B per lane, sixteen 1 KiB
//     pieces per image, four per wave; the swizzle is applied to the per-lane SOURCE chunk.
//   * One barrier per K-tile: wait for this wave's DMAs of tile t, barrier (every wave's DMAs of t have landed and
//     every wave's reads of t - 1 are done), read all of t's fragments, issue the DMAs of t + 1 into the other stage,
//     32 MFMAs.  The second block of the CU covers the barrier.
//   * Tails cost no branch in the K loop.  Each operand's buffer resource starts at the block's tile origin and ends
//     at the operand's true last element, so whole rows past the end (K-major: r >= R; MN-major: k >= K) are out of
//     range and the DMA writes zeros.  A chunk past the end of a row it starts in would wrap into the next row; those
//     lanes select an out-of-range offset instead (OOB): loop-invariant for an MN-major operand (r >= R), one compare
//     per DMA for a K-major one (k >= K, true only in the last K-tile).  Both operands are masked: 0 x NaN is NaN.
//   * The epilogue stores a lane's 4 columns only when m < M and n < N (N is a multiple of 8 and n of 4, so the four
//     are inside together); bias loads carry the same predicate.
//   * Split-K when the tile grid alone cannot fill the chip (narrow weight gradients, K = tokens): blockIdx.y owns
//     whole K-tiles, the last split is ragged, each split stores an fp32 slab and gemm_edge_reduce sums the slabs in
//     split order, then applies alpha, the accumulate or the bias.  No atomics: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PLX_API extern "C" __attribute__((visibility("default")))

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int BM = 128, BN = 128, BK = 64, NTH = 256, NW = 4;
constexpr int IMG = 16384;            // one operand's K-tile: 128 rows x 128 B (K-major) or 64 k-rows x 256 B (MN-major)
constexpr int STAGE = 2 * IMG;        // [A | B]
constexpr int LDS_BYTES = 2 * STAGE;  // 64 KiB: two blocks per CU
constexpr int PIECES = IMG / 1024 / NW;  // 1 KiB DMA pieces per wave per image

// An offset no resource of this file contains: every extent is at most 2^31 bytes.
constexpr uint32_t OOB = 0x80000000u;

// K-major rows (128 B): physical 16-B chunk = logical ^ kswz(row) (conflict-free ds_read_b128)
__device__ __forceinline__ int kswz(int row) { return (row >> 1) & 7; }
// MN-major k-rows (256 B): physical chunk = logical ^ tswz(row): the 8 k-rows one 32-lane half of a
// ds_read_b64_tr_b16 touches land on 8 disjoint 32-B bank windows
__device__ __forceinline__ int tswz(int row) { return 2 * ((row & 3) | (((row >> 3) & 1) << 2)); }

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

// `bytes`: the operand's extent from `base` (0 < bytes <= 2^31, a multiple of 16)
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

// Fragment addresses (gemm256's).  An MFMA fragment holds row r = c0 + (lane & 15) of an image (c0 16-aligned),
// k = 32 s + 8 (lane >> 4) + j.  K-major: kswz(c0 + fr) = kswz(fr), so the offset depends on (lane, s); tile t adds
// 16 rows (2048 B).  MN-major: tswz(kr) is unchanged by kr + 32 s and kr + 4, so (lane, t) fixes the offset; step s
// adds 32 k-rows (8192 B) and the fragment's second half 4 k-rows (1024 B).
template <bool KMAJ>
__device__ __forceinline__ int frag_off(int c0, int ts, int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  if (KMAJ) {  // ts = s
    return (c0 + fr) * 128 + (((ts * 4 + fq) ^ kswz(fr)) << 4);
  } else {     // ts = t; lane 4q + p of a 16-lane group addresses k-row q, columns c + 4p .. 4p + 3
    const int col = c0 + ts * 16 + 4 * (lane & 3);
    const int kr = 8 * fq + (fr >> 2);
    return kr * 256 + (((col >> 3) ^ tswz(kr)) << 4) + ((col >> 2) & 1) * 8;
  }
}

__device__ __forceinline__ bf16x8 ld_frag_k(const char* p) { return *(const bf16x8*)p; }

__device__ __forceinline__ bf16x8 ld_frag_t(const char* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p + 1024));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int V>
struct IC {
  static constexpr int value = V;
};

struct EdgeArgs {
  const __bf16* A;
  const __bf16* B;
  void* C;            // bf16 [M][ldc], or fp32 slabs [splits][M][N] when K is split
  int M, N, K, lda, ldb, ldc;
  int kt_per_split;   // K-tiles per blockIdx.y
  float alpha;
  const float* bias;  // fp32 [N] added after alpha in the bf16 epilogue, or null
  int group;          // M-tiles per tile group (tile_of)
};

// One operand's staging: the resource, and per DMA piece of this wave the lane's source offset at K-tile 0 with its
// swizzled chunk folded in.  R rows (M or N) of which the tile starts at r0; the block's K range starts at kbeg.
template <bool KMAJ>
struct Stager {
  __amdgpu_buffer_rsrc_t r;
  uint32_t off[PIECES];  // MN-major: OOB when the chunk's rows lie past R (loop-invariant)
  int klim[PIECES];      // K-major: the chunk is inside its row while 64 kt < klim
  uint32_t step;         // bytes per K-tile

  __device__ __forceinline__ Stager(const __bf16* X, int ld, int R, int K, int r0, int kbeg, int wave, int lane) {
    // elements from the tile origin to the operand's true last element + 1 (a multiple of 8; r0 < R, kbeg < K)
    const size_t rem = KMAJ ? (size_t)(R - 1 - r0) * ld + (K - kbeg) : (size_t)(K - 1 - kbeg) * ld + (R - r0);
    const size_t bytes = rem * 2;
    r = rsrc(KMAJ ? X + (size_t)r0 * ld + kbeg : X + (size_t)kbeg * ld + r0, bytes < OOB ? (uint32_t)bytes : OOB);
    step = KMAJ ? BK * 2 : (uint32_t)(BK * ld * 2);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int piece = wave + NW * i;
      if (KMAJ) {
        const int row = piece * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ kswz(row);
        off[i] = (uint32_t)((row * ld + chunk * 8) * 2);
        klim[i] = K - kbeg - chunk * 8;
      } else {
        const int kr = piece * 4 + (lane >> 4);
        const int chunk = (lane & 15) ^ tswz(kr);
        off[i] = r0 + chunk * 8 < R ? (uint32_t)((kr * ld + chunk * 8) * 2) : OOB;
        klim[i] = 0;
      }
    }
  }

  // DMA this wave's pieces of K-tile kt (relative to kbeg) into the image at `img`
  __device__ __forceinline__ void issue(int kt, char* img, int wave) const {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      // MN-major: OOB + kt * step stays out of range without wrapping (the host bounds K * ld * 2 below 2^31)
      const uint32_t o = KMAJ ? (kt * BK < klim[i] ? off[i] + (uint32_t)kt * step : OOB) : off[i] + (uint32_t)kt * step;
      glds(r, o, img + (wave + NW * i) * 1024);
    }
  }
};

// acc += the wave's 64 x 64 part of the tile at (m0, n0) over K-tiles [kt0, kt0 + nk)
template <bool AK, bool BKM>
__device__ __forceinline__ void edge_tile(const EdgeArgs& p, int m0, int n0, int kt0, int nk, f32x4 (&acc)[4][4],
                                          char* smem, int wave, int lane, int wm, int wn) {
  const Stager<AK> sa(p.A, p.lda, p.M, p.K, m0, kt0 * BK, wave, lane);
  const Stager<BKM> sb(p.B, p.ldb, p.N, p.K, n0, kt0 * BK, wave, lane);

  // per-lane fragment offsets inside an image (K-major: [s], MN-major: [t]); the rest of each address is an immediate
  int aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    aoff[i] = frag_off<AK>(wm * 64, AK ? (i & 1) : i, lane);
    boff[i] = frag_off<BKM>(wn * 64, BKM ? (i & 1) : i, lane);
  }

  auto step = [&](auto cb, int kt) {
    constexpr int CB = decltype(cb)::value;
    const char* ia = smem + CB * STAGE;
    const char* ib = ia + IMG;
    // this wave's DMAs of tile kt have landed and its earlier LDS reads are done; after the barrier, everyone's
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    bf16x8 fa[4][2], fb[4][2];  // [16-row tile][k step of 32]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        fa[t][s] = AK ? ld_frag_k(ia + aoff[s] + t * 2048) : ld_frag_t(ia + aoff[t] + s * 8192);
        fb[t][s] = BKM ? ld_frag_k(ib + boff[s] + t * 2048) : ld_frag_t(ib + boff[t] + s * 8192);
      }
    if (kt + 1 < nk) {  // the other stage: last read in step kt - 1, before the barrier above
      sa.issue(kt + 1, smem + (1 - CB) * STAGE, wave);
      sb.issue(kt + 1, smem + (1 - CB) * STAGE + IMG, wave);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[nt][s], fa[mt][s], acc[nt][mt], 0, 0, 0);
  };

  sa.issue(0, smem, wave);
  sb.issue(0, smem + IMG, wave);
  for (int kt = 0; kt < nk; kt += 2) {
    step(IC<0>{}, kt);
    if (kt + 1 < nk) step(IC<1>{}, kt + 1);
  }
}

// ACC: C += alpha * AB (bf16 read-modify-write); SLAB: write fp32 partials (split K)
template <bool AK, bool BKM, bool ACC, bool SLAB>
__global__ void __launch_bounds__(NTH, 2) gemm_edge_kernel(EdgeArgs p) {
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
  edge_tile<AK, BKM>(p, m0, n0, kt0, nk, acc, smem, wave, lane, wm, wn);

  // acc[nt][mt] is a 16 x 16 tile D[n][m]: m = lane & 15, n = 4 (lane >> 4) + j, j = 0..3
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
        v[0] = p.alpha * v[0] + __uint_as_float(o.x << 16);
        v[1] = p.alpha * v[1] + __uint_as_float(o.x & 0xffff0000u);
        v[2] = p.alpha * v[2] + __uint_as_float(o.y << 16);
        v[3] = p.alpha * v[3] + __uint_as_float(o.y & 0xffff0000u);
      } else {
        v = v * p.alpha + bias;
      }
      *(uint2*)dst = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

// C (bf16, ldc) = alpha * sum over splits (in split order) of the fp32 slabs (+ bias) (+ C when accumulating);
// 8 elements per thread (N is a multiple of 8: a thread's 8 stay in one row)
template <bool ACC>
__global__ void __launch_bounds__(256) gemm_edge_reduce(const float* __restrict__ ws, __bf16* __restrict__ C, int M,
                                                        int N, int ldc, int splits, float alpha,
                                                        const float* __restrict__ bias) {
  const size_t i8 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i8 >= (size_t)M * N / 8) return;
  const size_t e = i8 * 8;
  const int m = (int)(e / N), n = (int)(e % N);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  const size_t slab = (size_t)M * N;
  for (int k = 0; k < splits; ++k) {
    const f32x4* src = (const f32x4*)(ws + k * slab + e);
    s0 += src[0];
    s1 += src[1];
  }
  s0 *= alpha;
  s1 *= alpha;
  if (bias != nullptr) {
    s0 += *(const f32x4*)(bias + n);
    s1 += *(const f32x4*)(bias + n + 4);
  }
  __bf16* dst = C + (size_t)m * ldc + n;
  if (ACC) {
    const uint4 o = *(const uint4*)dst;
    s0[0] += __uint_as_float(o.x << 16);
    s0[1] += __uint_as_float(o.x & 0xffff0000u);
    s0[2] += __uint_as_float(o.y << 16);
    s0[3] += __uint_as_float(o.y & 0xffff0000u);
    s1[0] += __uint_as_float(o.z << 16);
    s1[1] += __uint_as_float(o.z & 0xffff0000u);
    s1[2] += __uint_as_float(o.w << 16);
    s1[3] += __uint_as_float(o.w & 0xffff0000u);
  }
  uint4 packed;
  packed.x = pack_bf16x2(s0[0], s0[1]);
  packed.y = pack_bf16x2(s0[2], s0[3]);
  packed.z = pack_bf16x2(s1[0], s1[1]);
  packed.w = pack_bf16x2(s1[2], s1[3]);
  *(uint4*)dst = packed;
}

template <bool AK, bool BKM, bool ACC, bool SLAB>
int launch(const EdgeArgs& a, int splits, hipStream_t st) {
  auto k = gemm_edge_kernel<AK, BKM, ACC, SLAB>;
  static const int attr =
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess ? 0 : -4;
  if (attr) return attr;
  const dim3 grid(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), splits);
  hipLaunchKernelGGL(k, grid, dim3(NTH), LDS_BYTES, st, a);
  return 0;
}

template <bool AK, bool BKM>
int dispatch(const EdgeArgs& a, int splits, int accumulate, hipStream_t st) {
  if (splits > 1) return launch<AK, BKM, false, true>(a, splits, st);
  return accumulate ? launch<AK, BKM, true, false>(a, 1, st) : launch<AK, BKM, false, false>(a, 1, st);
}

constexpr int kSplitTarget = 512;  // blocks the split-K planner aims for: two per CU of a 256-CU chip
constexpr int kGroup = 4;

bool shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 8 == 0 && N % 8 == 0 && K % 8 == 0; }

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
PLX_API int plx_gemm_edge_splits(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return 0;
  const int kps = plan_kt_per_split(M, N, K);
  return ((K + BK - 1) / BK + kps - 1) / kps;
}

// fp32 workspace floats the launch needs (0 when K is not split, -1 for a shape the kernel does not take)
PLX_API long long plx_gemm_edge_ws(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return -1;
  const int s = plx_gemm_edge_splits(M, N, K);
  return s > 1 ? (long long)s * M * N : 0;
}

PLX_API int plx_gemm_edge_tile() { return BM; }

// C[M][N] (bf16, ldc) = alpha * A . B (+ bias[n]) (+ C when accumulate), layouts per a_kmajor / b_kmajor (see the
// file header); M, N, K multiples of 8.  bias: fp32 [N], 16-byte aligned, or null (not combined with accumulate).
// ws: plx_gemm_edge_ws(M, N, K) floats, 16-byte aligned (may be null when that is 0).
// Returns 0, or < 0 on a shape / layout the kernel does not take (nothing launched).
PLX_API int plx_gemm_edge(const void* A, const void* B, void* C, void* ws, int M, int N, int K, int lda, int ldb, int ldc,
                          int a_kmajor, int b_kmajor, float alpha, int accumulate, const float* bias, void* stream) {
  if (!shape_ok(M, N, K)) return -1;
  if (bias != nullptr && (accumulate || (uintptr_t)bias % 16)) return -1;
  if (lda % 8 || ldb % 8 || ldc % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)C % 16) return -1;
  if (lda < (a_kmajor ? K : M) || ldb < (b_kmajor ? K : N) || ldc < N) return -1;
  // the largest byte offset a block forms relative to its tile origin, tails included (it must stay below 2^31)
  const long long aspan = a_kmajor ? ((long long)BM * lda + K + BK) * 2 : ((long long)(K + BK) * lda + BM) * 2;
  const long long bspan = b_kmajor ? ((long long)BN * ldb + K + BK) * 2 : ((long long)(K + BK) * ldb + BN) * 2;
  if (aspan >= 0x7ffffff0LL || bspan >= 0x7ffffff0LL) return -2;
  const int kps = plan_kt_per_split(M, N, K);
  const int splits = ((K + BK - 1) / BK + kps - 1) / kps;
  if (splits > 1 && (!ws || (uintptr_t)ws % 16)) return -5;
  EdgeArgs a{(const __bf16*)A, (const __bf16*)B, splits > 1 ? ws : C, M, N, K, lda, ldb, ldc, kps, alpha, bias, kGroup};
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (a_kmajor && b_kmajor) rc = dispatch<true, true>(a, splits, accumulate, st);
  else if (a_kmajor) rc = dispatch<true, false>(a, splits, accumulate, st);
  else if (b_kmajor) rc = dispatch<false, true>(a, splits, accumulate, st);
  else rc = dispatch<false, false>(a, splits, accumulate, st);
  if (rc) return rc;
  if (splits > 1) {
    const size_t total8 = (size_t)M * N / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256));
    if (accumulate)
      hipLaunchKernelGGL(gemm_edge_reduce<true>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C, M, N, ldc, splits,
                         alpha, (const float*)nullptr);
    else
      hipLaunchKernelGGL(gemm_edge_reduce<false>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C, M, N, ldc, splits,
                         alpha, bias);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
