// Grouped bf16 GEMM for mixture-of-experts feed-forwards on MI355X (gfx950): E problems in one launch whose sizes are
// DEVICE data.  `offs` is an int32 [E + 1] table in device memory; segment e is rows offs[e] .. offs[e + 1] of a
// packed [P][.] activation (the tokens routed to expert e).  P, E, N, K are host integers; no launch parameter, grid
// size or workspace depends on the table's contents, nothing is read back, there are no atomics: the launch is
// capturable and the same inputs give bitwise the same outputs.
//
//   rows mode    C[p][n]    = sum_k A[p][k] B_e(n, k)           for p in segment e       (forward, data gradient)
//   reduce mode  C_e[m][n]  = sum_{p in segment e} A[p][m] B[p][n]                        (weight gradient)
//
// The tile is csrc/gemm_edge.hip's: 128 x 128 x 64, 256 threads = 4 waves as 2 (M) x 2 (N), each wave 4 x 4 tiles of
// v_mfma_f32_16x16x32_bf16, two LDS stages of [A 16 KiB | B 16 KiB], staged by buffer-resource LDS-DMA (16 B per
// lane, the XOR swizzle applied to the per-lane source chunk), one barrier per K-tile.  A segment boundary is a tail
// in the middle of the tensor, and tails cost what they cost there: every operand's buffer resource starts at the
// tile origin and ENDS AT THE SEGMENT'S last element, so rows of the next expert are out of range and the DMA stages
// zeros for them.
//
//   * Rows mode.  M-tiles never cross a segment: expert e owns ceil(len_e / 128) of them, at most P / 128 + E in all,
//     and the grid is that worst case times ceil(N / 128).  Every wave scans the table itself (E <= 64: one lane per
//     expert, a 6-step shuffle prefix sum of the tile counts, one ballot to find the owner), so a workgroup knows its
//     (expert, M-tile, N-tile) -- or that its id is past the real tile count, and exits -- before its first barrier
//     and without LDS.  Ids are expert-major, and inside an expert they walk the M-tiles of one N-column before the
//     next column; the XCD remap (over the REAL tile count) puts consecutive ids on one XCD, so neighbours share the
//     expert's 128-row B panel in that XCD's L2.  The epilogue stores row m only when m < offs[e + 1].
//   * Reduce mode.  The grid is E x ceil(M / 128) x ceil(N / 128), fixed.  Both operands are MN-major with the packed
//     tokens as k-rows; expert e walks the K range [offs[e], offs[e + 1]) whole, in order (no split-K: one summation
//     order).  Start and length are arbitrary: the resource origin is row offs[e], its end row offs[e + 1].  An empty
//     expert issues no DMA at all and stores exact zeros.
//   * Every offset is clamped to [0, P] and a segment's length to >= 0: whatever the table holds, no address leaves
//     the operands.
//
// plx_moe_gather / plx_moe_combine / plx_moe_gate_grad are the routing passes around the GEMMs (packed row <- token
// row, token row <- gated sum of its k packed rows in fixed order, and the gate gradient).
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
constexpr int MAX_E = 64;             // one lane per expert in the table scan

// An offset no resource of this file contains: every extent is below 2^31 bytes.
constexpr uint32_t OOB = 0x80000000u;

// K-major rows (128 B): physical 16-B chunk = logical ^ kswz(row) (conflict-free ds_read_b128)
__device__ __forceinline__ int kswz(int row) { return (row >> 1) & 7; }
// MN-major k-rows (256 B): physical chunk = logical ^ tswz(row): the 8 k-rows one 32-lane half of a
// ds_read_b64_tr_b16 touches land on 8 disjoint 32-B bank windows
__device__ __forceinline__ int tswz(int row) { return 2 * ((row & 3) | (((row >> 3) & 1) << 2)); }

// workgroups are dealt round-robin to the 8 XCDs: logical ids [base, base + share) of `n` go to one XCD
__device__ __forceinline__ int xcd_remap(int bid, int n) {
  const int xcd = bid & 7, q = n >> 3, r = n & 7;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (bid >> 3);
}

__device__ __forceinline__ void glds(__amdgpu_buffer_rsrc_t r, uint32_t off, void* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)l, 16, off, 0, 0, 0);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)b) << 16);
}

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// Fragment addresses inside an image.  An MFMA fragment holds row r = c0 + (lane & 15), k = 32 s + 8 (lane >> 4) + j.
// K-major: the offset depends on (lane, s), tile t adds 16 rows (2048 B).  MN-major: (lane, t) fixes it, step s adds
// 32 k-rows (8192 B) and the fragment's second half 4 k-rows (1024 B).
template <bool KMAJ>
__device__ __forceinline__ int frag_off(int c0, int ts, int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  if (KMAJ) {
    return (c0 + fr) * 128 + (((ts * 4 + fq) ^ kswz(fr)) << 4);
  } else {
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

// One operand's staging for one tile.  `origin` is the tile's first element; the operand (as this tile may see it)
// has `rows` more rows / columns of the MN dimension and `kext` more of the K dimension from there, both > 0:
//   K-major  X[r][k], ld >= kext: the extent ends after row rows - 1, so rows past it stage zeros; a chunk at
//            k >= kext would wrap into the next row and selects OOB instead (true only in the last K-tile);
//   MN-major X[k][r]: the extent ends after k-row kext - 1; chunks at r >= rows select OOB (loop-invariant).
// Both sides of a product are masked: 0 x NaN is NaN.
template <bool KMAJ>
struct Stager {
  __amdgpu_buffer_rsrc_t r;
  uint32_t off[PIECES];
  int klim[PIECES];
  uint32_t step;  // bytes per K-tile

  __device__ __forceinline__ Stager(const __bf16* origin, int ld, int rows, int kext, int wave, int lane) {
    // no tile reads past its 128 rows: with the host's span checks the extent (a multiple of 16 bytes) is below 2^31
    const int tr = min(rows, BM);
    const size_t rem = KMAJ ? (size_t)(tr - 1) * ld + kext : (size_t)(kext - 1) * ld + tr;
    r = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(origin), 0, (int)(rem * 2), 0x00020000);
    step = KMAJ ? BK * 2 : (uint32_t)(BK * ld * 2);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int piece = wave + NW * i;
      if (KMAJ) {
        const int row = piece * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ kswz(row);
        off[i] = (uint32_t)((row * ld + chunk * 8) * 2);
        klim[i] = kext - chunk * 8;
      } else {
        const int kr = piece * 4 + (lane >> 4);
        const int chunk = (lane & 15) ^ tswz(kr);
        off[i] = chunk * 8 < rows ? (uint32_t)((kr * ld + chunk * 8) * 2) : OOB;
        klim[i] = 0;
      }
    }
  }

  // DMA this wave's pieces of K-tile kt into the image at `img`
  __device__ __forceinline__ void issue(int kt, char* img, int wave) const {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      // MN-major: OOB + kt * step stays out of range without wrapping (the host bounds (P + 64) * ld * 2 below 2^31)
      const uint32_t o = KMAJ ? (kt * BK < klim[i] ? off[i] + (uint32_t)kt * step : OOB) : off[i] + (uint32_t)kt * step;
      glds(r, o, img + (wave + NW * i) * 1024);
    }
  }
};

// acc += the wave's 64 x 64 part of one tile over K-tiles [0, nk), nk >= 1 (a caller with nothing to add does not call:
// tile 0 is issued unconditionally)
template <bool AK, bool BKM>
__device__ __forceinline__ void mainloop(const Stager<AK>& sa, const Stager<BKM>& sb, int nk, f32x4 (&acc)[4][4],
                                         char* smem, int wave, int lane, int wm, int wn) {
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

__device__ __forceinline__ void zero(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// segment e as [lo, lo + len) inside [0, P], whatever the table holds
__device__ __forceinline__ void segment(const int* __restrict__ offs, int e, int P, int& lo, int& len) {
  lo = clampi(offs[e], 0, P);
  len = max(clampi(offs[e + 1], 0, P) - lo, 0);
}

struct RowsArgs {
  const __bf16* A;    // [P][lda], K-major
  const __bf16* B;    // expert e at B + e * stride_b: [N][ldb] (K-major) or [K][ldb] (MN-major)
  __bf16* C;          // [P][ldc]
  const int* offs;    // [E + 1], device
  int P, E, N, K, lda, ldb, ldc;
  long long stride_b;
};

template <bool BKM>
__global__ void __launch_bounds__(NTH, 2) grouped_rows_kernel(RowsArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (p.N + BN - 1) / BN;

  // the table scan, by every wave for itself: lane e holds expert e's segment and its tile count
  int lo = 0, len = 0;
  if (lane < p.E) segment(p.offs, lane, p.P, lo, len);
  const int mine = ((len + BM - 1) / BM) * ntn;
  int incl = mine;  // inclusive prefix sum over the lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const int total = __shfl(incl, 63, 64);
  const int bid = blockIdx.x;
  if (bid >= total) return;  // uniform over the workgroup, before any barrier
  const int id = xcd_remap(bid, total);
  const unsigned long long owners = __ballot(incl > id);  // id < total: not empty
  const int e = __builtin_amdgcn_readfirstlane(__ffsll((long long)owners) - 1);
  const int e_lo = __builtin_amdgcn_readfirstlane(__shfl(lo, e, 64));
  const int e_len = __builtin_amdgcn_readfirstlane(__shfl(len, e, 64));
  const int local = id - __builtin_amdgcn_readfirstlane(__shfl(incl - mine, e, 64));
  const int mt_e = (e_len + BM - 1) / BM;
  const int tm = local % mt_e, tn = local / mt_e;  // the M-tiles of one B panel are neighbours
  const int m0 = e_lo + tm * BM, m_end = e_lo + e_len, n0 = tn * BN;

  f32x4 acc[4][4];  // [n tile][m tile] of the wave's 64 x 64
  zero(acc);
  {
    const Stager<true> sa(p.A + (size_t)m0 * p.lda, p.lda, m_end - m0, p.K, wave, lane);
    const __bf16* Be = p.B + (size_t)e * p.stride_b;
    const Stager<BKM> sb(BKM ? Be + (size_t)n0 * p.ldb : Be + n0, p.ldb, p.N - n0, p.K, wave, lane);
    mainloop<true, BKM>(sa, sb, (p.K + BK - 1) / BK, acc, smem, wave, lane, wm, wn);
  }

  // acc[nt][mt] is a 16 x 16 tile D[n][m]: m = lane & 15, n = 4 (lane >> 4) + j, j = 0..3
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = n0 + wn * 64 + nt * 16 + 4 * fq;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = m0 + wm * 64 + mt * 16 + fr;
      if (m >= m_end || n >= p.N) continue;
      const f32x4 v = acc[nt][mt];
      *(uint2*)(p.C + (size_t)m * p.ldc + n) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

struct WgradArgs {
  const __bf16* A;  // [P][lda], the M dimension contiguous
  const __bf16* B;  // [P][ldb], the N dimension contiguous
  void* C;          // [E][M][N], bf16 or fp32
  const int* offs;
  int P, E, M, N, lda, ldb;
};

template <bool F32>
__global__ void __launch_bounds__(NTH, 2) grouped_wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  const int per = ntm * ntn;
  const int id = xcd_remap(blockIdx.x, gridDim.x);  // expert-major: an expert's tiles share its token rows in L2
  const int e = id / per, local = id - e * per;
  const int tm = local % ntm, tn = local / ntm;
  const int m0 = tm * BM, n0 = tn * BN;
  int lo, len;
  segment(p.offs, e, p.P, lo, len);
  lo = __builtin_amdgcn_readfirstlane(lo);
  len = __builtin_amdgcn_readfirstlane(len);

  f32x4 acc[4][4];
  zero(acc);
  if (len > 0) {  // an empty expert has no K-tile: no resource, no DMA, no barrier (uniform over the workgroup)
    const Stager<false> sa(p.A + (size_t)lo * p.lda + m0, p.lda, p.M - m0, len, wave, lane);
    const Stager<false> sb(p.B + (size_t)lo * p.ldb + n0, p.ldb, p.N - n0, len, wave, lane);
    mainloop<false, false>(sa, sb, (len + BK - 1) / BK, acc, smem, wave, lane, wm, wn);
  }

  const int fr = lane & 15, fq = lane >> 4;
  const size_t base = (size_t)e * p.M * p.N;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int n = n0 + wn * 64 + nt * 16 + 4 * fq;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int m = m0 + wm * 64 + mt * 16 + fr;
      if (m >= p.M || n >= p.N) continue;
      const f32x4 v = acc[nt][mt];
      const size_t at = base + (size_t)m * p.N + n;
      if (F32) *(f32x4*)((float*)p.C + at) = v;
      else *(uint2*)((__bf16*)p.C + at) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
  }
}

// out[p][:] = (scale ? scale[p] : 1) * x[idx[p]][:], rows of D bf16 as 16-byte vectors (D % 8 == 0); idx clamped to
// [0, T).  The forward gather (no scale) and the combine's backward (scale = the packed gates).
__global__ void __launch_bounds__(256) moe_gather_kernel(const uint4* __restrict__ x, const int* __restrict__ idx,
                                                         const float* __restrict__ scale, uint4* __restrict__ out,
                                                         int P, int T, int D8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)P * D8) return;
  const int prow = (int)(i / D8), c = (int)(i - (size_t)prow * D8);
  uint4 v = x[(size_t)clampi(idx[prow], 0, T - 1) * D8 + c];
  if (scale != nullptr) {
    const float g = scale[prow];
    v.x = pack_bf16x2(g * bf_lo(v.x), g * bf_hi(v.x));
    v.y = pack_bf16x2(g * bf_lo(v.y), g * bf_hi(v.y));
    v.z = pack_bf16x2(g * bf_lo(v.z), g * bf_hi(v.z));
    v.w = pack_bf16x2(g * bf_lo(v.w), g * bf_hi(v.w));
  }
  out[i] = v;
}

// y[t][:] = sum_j (gate ? gate[t][j] : 1) * yp[slot[t][j]][:], j = 0 .. k - 1 in that order, fp32 sum, bf16 out
__global__ void __launch_bounds__(256) moe_combine_kernel(const uint4* __restrict__ yp, const int* __restrict__ slot,
                                                          const float* __restrict__ gate, uint4* __restrict__ y,
                                                          int T, int k, int P, int D8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)T * D8) return;
  const int t = (int)(i / D8), c = (int)(i - (size_t)t * D8);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    const uint4 v = yp[(size_t)clampi(slot[(size_t)t * k + j], 0, P - 1) * D8 + c];
    const float g = gate != nullptr ? gate[(size_t)t * k + j] : 1.f;
    s[0] += g * bf_lo(v.x), s[1] += g * bf_hi(v.x), s[2] += g * bf_lo(v.y), s[3] += g * bf_hi(v.y);
    s[4] += g * bf_lo(v.z), s[5] += g * bf_hi(v.z), s[6] += g * bf_lo(v.w), s[7] += g * bf_hi(v.w);
  }
  y[i] = make_uint4(pack_bf16x2(s[0], s[1]), pack_bf16x2(s[2], s[3]), pack_bf16x2(s[4], s[5]), pack_bf16x2(s[6], s[7]));
}

// dgate[t][j] = <dy[t], yp[slot[t][j]]>: one wave per (t, j), lanes stride the row, a fixed butterfly sums them
__global__ void __launch_bounds__(256) moe_gate_grad_kernel(const uint4* __restrict__ dy, const uint4* __restrict__ yp,
                                                            const int* __restrict__ slot, float* __restrict__ dgate,
                                                            int T, int k, int P, int D8) {
  const int lane = threadIdx.x & 63;
  const size_t pair = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (size_t)T * k) return;  // uniform over the wave
  const uint4* a = dy + (pair / k) * D8;
  const uint4* b = yp + (size_t)clampi(slot[pair], 0, P - 1) * D8;
  float s = 0.f;
  for (int c = lane; c < D8; c += 64) {
    const uint4 u = a[c], v = b[c];
    s += bf_lo(u.x) * bf_lo(v.x) + bf_hi(u.x) * bf_hi(v.x) + bf_lo(u.y) * bf_lo(v.y) + bf_hi(u.y) * bf_hi(v.y) +
         bf_lo(u.z) * bf_lo(v.z) + bf_hi(u.z) * bf_hi(v.z) + bf_lo(u.w) * bf_lo(v.w) + bf_hi(u.w) * bf_hi(v.w);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) dgate[pair] = s;
}

template <typename K>
int set_lds(K k) {
  return hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess ? 0 : -4;
}

bool aligned(const void* p) { return p != nullptr && (uintptr_t)p % 16 == 0; }

constexpr long long kSpan = 0x7ffffff0LL;

// rows mode: which of the arguments the kernel takes (0), else < 0
int rows_check(const void* A, const void* B, const void* C, const void* offs, int P, int E, int N, int K, int lda, int ldb,
               int ldc, long long stride_b, int b_kmajor) {
  if (P <= 0 || E <= 0 || E > MAX_E || N <= 0 || K <= 0 || N % 8 || K % 8) return -1;
  if (!aligned(A) || !aligned(B) || !aligned(C) || !offs || (uintptr_t)offs % 4) return -1;
  if (lda % 8 || ldb % 8 || ldc % 8 || stride_b % 8 || stride_b < 0) return -1;
  if (lda < K || ldb < (b_kmajor ? K : N) || ldc < N) return -1;
  // the largest byte offset a block forms from its tile origin, tails included, must stay below 2^31
  const long long aspan = ((long long)BM * lda + K + BK) * 2;
  const long long bspan = b_kmajor ? ((long long)BN * ldb + K + BK) * 2 : ((long long)(K + BK) * ldb + BN) * 2;
  if (aspan >= kSpan || bspan >= kSpan) return -2;
  if (((long long)(P / BM) + E) * ((N + BN - 1) / BN) >= 0x7fffffffLL) return -2;
  return 0;
}

int wgrad_check(const void* A, const void* B, const void* C, const void* offs, int P, int E, int M, int N, int lda,
                int ldb) {
  if (P <= 0 || E <= 0 || E > MAX_E || M <= 0 || N <= 0 || M % 8 || N % 8) return -1;
  if (!aligned(A) || !aligned(B) || !aligned(C) || !offs || (uintptr_t)offs % 4) return -1;
  if (lda % 8 || ldb % 8 || lda < M || ldb < N) return -1;
  const long long aspan = ((long long)(P + BK) * lda + BM) * 2, bspan = ((long long)(P + BK) * ldb + BN) * 2;
  if (aspan >= kSpan || bspan >= kSpan) return -2;
  if ((long long)E * ((M + BM - 1) / BM) * ((N + BN - 1) / BN) >= 0x7fffffffLL) return -2;
  return 0;
}

}  // namespace

PLX_API int plx_gemm_grouped_tile() { return BM; }

// workgroups a rows-mode launch starts: the worst case over every table (a function of the host integers alone)
PLX_API long long plx_gemm_grouped_rows_blocks(int P, int E, int N) {
  if (P <= 0 || E <= 0 || E > MAX_E || N <= 0) return -1;
  return ((long long)(P / BM) + E) * ((N + BN - 1) / BN);
}

// The shape check of a grouped linear with weights [E][N][K] over P packed rows of contiguous operands: 0 when
// plx_gemm_grouped_rows takes its forward and data gradient (reduce = 0) / plx_gemm_grouped_wgrad its [E][N][K] weight
// gradient (reduce = 1), else < 0.  The launchers repeat it on their own arguments, pointers included.
PLX_API int plx_gemm_grouped_check(int P, int E, int N, int K, int reduce) {
  static const __attribute__((aligned(16))) char dummy[16] = {0};
  if (reduce) return wgrad_check(dummy, dummy, dummy, dummy, P, E, N, K, N, K);
  const int kk = rows_check(dummy, dummy, dummy, dummy, P, E, N, K, K, K, N, (long long)N * K, 1);
  return kk ? kk : rows_check(dummy, dummy, dummy, dummy, P, E, K, N, N, K, K, (long long)N * K, 0);
}

// Rows mode: for p in [offs[e], offs[e + 1]), C[p][n] = sum_k A[p][k] B_e(n, k), B_e = B + e * stride_b elements, stored
// [N][ldb] when b_kmajor else [K][ldb].  Rows of C outside every segment are not written.  Returns 0, or < 0 on
// arguments the kernel does not take (nothing launched).
PLX_API int plx_gemm_grouped_rows(const void* A, const void* B, void* C, const void* offs, int P, int E, int N, int K,
                                  int lda, int ldb, int ldc, long long stride_b, int b_kmajor, void* stream) {
  const int rc = rows_check(A, B, C, offs, P, E, N, K, lda, ldb, ldc, stride_b, b_kmajor);
  if (rc) return rc;
  static const int attr = set_lds(grouped_rows_kernel<true>) | set_lds(grouped_rows_kernel<false>);
  if (attr) return -4;
  const RowsArgs a{(const __bf16*)A, (const __bf16*)B, (__bf16*)C, (const int*)offs, P, E, N, K, lda, ldb, ldc, stride_b};
  const dim3 grid((unsigned)plx_gemm_grouped_rows_blocks(P, E, N));
  if (b_kmajor) hipLaunchKernelGGL(grouped_rows_kernel<true>, grid, dim3(NTH), LDS_BYTES, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(grouped_rows_kernel<false>, grid, dim3(NTH), LDS_BYTES, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// Reduce mode: C_e[m][n] = sum over p in [offs[e], offs[e + 1]) of A[p][m] B[p][n], C_e = C + e * M * N (bf16, or fp32
// when out_f32); an empty segment writes zeros.
PLX_API int plx_gemm_grouped_wgrad(const void* A, const void* B, void* C, const void* offs, int P, int E, int M, int N,
                                   int lda, int ldb, int out_f32, void* stream) {
  const int rc = wgrad_check(A, B, C, offs, P, E, M, N, lda, ldb);
  if (rc) return rc;
  static const int attr = set_lds(grouped_wgrad_kernel<true>) | set_lds(grouped_wgrad_kernel<false>);
  if (attr) return -4;
  const WgradArgs a{(const __bf16*)A, (const __bf16*)B, C, (const int*)offs, P, E, M, N, lda, ldb};
  const dim3 grid((unsigned)(E * ((M + BM - 1) / BM) * ((N + BN - 1) / BN)));
  if (out_f32) hipLaunchKernelGGL(grouped_wgrad_kernel<true>, grid, dim3(NTH), LDS_BYTES, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(grouped_wgrad_kernel<false>, grid, dim3(NTH), LDS_BYTES, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// out[p] = (scale ? scale[p] : 1) * x[idx[p]]: x [T][D], out [P][D] bf16, idx int32 [P], scale fp32 [P] or null
PLX_API int plx_moe_gather(const void* x, const void* idx, const void* scale, void* out, int P, int T, int D,
                           void* stream) {
  if (P <= 0 || T <= 0 || D <= 0 || D % 8 || !aligned(x) || !aligned(out) || !idx) return -1;
  const size_t n = (size_t)P * (D / 8);
  hipLaunchKernelGGL(moe_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)x, (const int*)idx, (const float*)scale, (uint4*)out, P, T, D / 8);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// y[t] = sum_j (gate ? gate[t][j] : 1) * yp[slot[t][j]]: yp [P][D], y [T][D] bf16, slot int32 [T][k], gate fp32 [T][k]
PLX_API int plx_moe_combine(const void* yp, const void* slot, const void* gate, void* y, int T, int k, int P, int D,
                            void* stream) {
  if (P <= 0 || T <= 0 || k <= 0 || D <= 0 || D % 8 || !aligned(yp) || !aligned(y) || !slot) return -1;
  const size_t n = (size_t)T * (D / 8);
  hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)yp, (const int*)slot, (const float*)gate, (uint4*)y, T, k, P, D / 8);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// dgate[t][j] = <dy[t], yp[slot[t][j]]> (fp32 [T][k])
PLX_API int plx_moe_gate_grad(const void* dy, const void* yp, const void* slot, void* dgate, int T, int k, int P, int D,
                              void* stream) {
  if (P <= 0 || T <= 0 || k <= 0 || D <= 0 || D % 8 || !aligned(dy) || !aligned(yp) || !slot || !dgate) return -1;
  const size_t pairs = (size_t)T * k;
  hipLaunchKernelGGL(moe_gate_grad_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)dy, (const uint4*)yp, (const int*)slot, (float*)dgate, T, k, P, D / 8);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
