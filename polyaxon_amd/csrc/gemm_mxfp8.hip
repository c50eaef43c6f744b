// MXFP8 (OCP microscaling) GEMM for the language-model linears on MI355X (gfx950): gemm_fp8.hip's tile, staging and
// split-K with one E8M0 scale per 32 K-values of every operand row, applied by the MFMA itself
// (v_mfma_scale_f32_16x16x128_f8f6f4).  A block's scale depends on its 32 values only, so the cast computes it in the
// read that converts the data: no amax launch, no atomics, no state words.
//
//   plx_mxfp8_cast  bf16 [R][C] -> FP8 q [R][C] with scales sq (blocks along C) and FP8 qt [C][R] with scales sqt
//                   (blocks along R), one read.  The transposed copy is quantised from the bf16 values with its own
//                   block maxima over 32 rows; it is not a byte transpose of q.  R, C multiples of 32.
//   plx_gemm_mxfp8  C[M][N] = alpha * sum_k (A[m][k] 2^(sA - 127)) (B[n][k] 2^(sB - 127))  (+ C) (+ bias[n]) (second
//                   store: gelu_tanh), C bf16 (ldc), A (E4M3 or E5M2) and B (E4M3) K-MAJOR bytes.  M, N multiples of
//                   16, K a multiple of 32.
//
// Scales.  Block amax a -> 2^e = 2^floor(log2(FMAX / a)), e <= 126 (1 when a is 0 or not finite: ops/fp8.py
// scale_for), element = cvt(clamp(x 2^e, +-FMAX)), scale byte = 127 - e in [1, 247]: never 255, E8M0's NaN.
// Layout: for an operand [rows][K] a uint32 [ceil(K / 128)][rows] array; byte j of word [kt][row] belongs to K-block
// 4 kt + j; bytes of blocks at k >= K are 127.  For one K-tile the 16 lanes of a fragment's row group read 64
// contiguous bytes, and nothing depends on K / 32 being a multiple of 4.
//
// The cast.  A block of 256 threads converts a 64 x 64 tile (2 x 2 MX blocks each way; 8 KiB of LDS; 2-byte scale
// stores -- the 128 x 128 tile with whole scale words would leave a 768 x 768 weight 36 blocks for 256 CUs).
//   * Row pass p: thread (r = 32 p + tid / 8, c8 = tid & 7) loads 8 bf16 (16 B).  The 4 lanes c8 & ~3 .. + 3 hold one
//     MX block of the row and are one DPP quad: two quad_perm max steps give every lane the block's amax.  The lane
//     scales, clamps and converts its 8 values and stores their 8 bytes; lane c8 = 0 fetches the second block's byte
//     from lane + 4 and stores both as one 2-byte word.
//   * LDS tile: the raw bf16, 64 rows of 128 B, physical 16-byte chunk = c8 ^ (row >> 3).  A ds_write_b128 is served
//     16 lanes at a time: 2 whole rows = 256 contiguous bytes, each of the 64 banks once whatever the permutation
//     inside a row.
//   * Column pass i: thread (c = 32 i + tid / 8, g = tid & 7) reads column c of rows 8 g .. 8 g + 7 with 8
//     ds_read_u16.  At step j the wave's 8 row groups read rows 8 g + j: unswizzled they would share 4 banks (row
//     stride 128 B = 32 banks, 8 g + j all of one parity); the swizzle puts group g in chunk (c >> 3) ^ g, 8 different
//     chunks = 32 different banks, and the 8 lanes of one group share 4 words (a broadcast).  The 4 lanes g & ~3 ..
//     + 3 hold one MX block of the column -- again a quad -- so the same two DPP steps give its amax; each lane
//     stores 8 transposed bytes, 8 lanes 64 contiguous bytes.
//
// The GEMM keeps gemm_fp8.hip's design: tile 128 x 128 x 128, 256 threads = 4 waves as 2 (M) x 2 (N), two blocks per
// CU, each wave 4 x 4 tiles of the 16x16x128 MFMA (MFMA A operand = B's rows, B operand = A's rows); 2 stages x
// (A 16 KiB + B 16 KiB) of LDS filled by buffer-resource LDS-DMA with the chunk swizzle on the source side (bank
// argument: gemm_fp8.hip); one barrier per K-tile; resources that end at the true last byte, so tails stage zeros;
// deterministic fp32-slab split-K with a reduce kernel.  New is the scale path:
//   * The scaled MFMA fixes which k a register holds, which the unscaled kernel never had to know: lane (fr, fq)'s
//     registers 0-3 are k = 16 fq .. 16 fq + 15 of row fr and its registers 4-7 are k = 64 + 16 fq .. + 15, and MX
//     block b (k = 32 b .. 32 b + 31) of row fr takes its scale from lane fr + 16 b.  (Measured: with gemm_fp8.hip's
//     fragment, bytes 32 fq .. 32 fq + 31 per lane, the 16 x 16 x 32 case returned sum(k < 16) 2^(sA + sB - 254) +
//     sum(16 <= k < 32) 2^0 -- the lane's second half scaled by block 2's pad bytes.)  So a fragment is logical
//     chunks fq and 4 + fq of the K-tile row -- gemm_fp8.hip's bank argument holds for any fixed logical chunk -- and
//     lane (fr, fq) supplies the scale of block fq.
//   * Per K-tile the lane loads, for each of its 4 + 4 row-tiles, the word [kt][row] global -> VGPR through a resource
//     that ends at the array's true last byte (rows past the edge select an out-of-range offset and read 0 = 2^-127,
//     times staged zeros: 0, not NaN), shifts byte fq down to byte 0 (one v_lshrrev: op_sel is an immediate and
//     cannot vary by lane) and feeds the word as the scale operand with op_sel 0.
//   * The words of K-tile kt + 1 are requested right after its DMAs are issued and are first used after the next
//     tile's s_waitcnt vmcnt(0), which the DMAs need anyway.
//   * A K split starts at a whole K-tile, so scale words never straddle splits.
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

// ------------------------------------------------------------------------------------------------ the cast
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

// max over the 4 lanes of a DPP quad (quad_perm [1,0,3,2], then [2,3,0,1]); every lane of the wave is active
__device__ __forceinline__ unsigned quad_max(unsigned m) {
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false));
  return max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false));
}

// the block's scale 2^e and its E8M0 byte 127 - e from the bit pattern of its amax (|x| as fp32 bits, which order
// like the values, NaN above inf)
template <int FMT>
__device__ __forceinline__ float block_scale(unsigned bits, unsigned& byte) {
  byte = 127;
  if (bits == 0 || bits >= 0x7f800000u) return 1.f;
  const float q = fmax_of(FMT) / __uint_as_float(bits);  // IEEE division; its exponent is floor(log2 q)
  const int e = min((int)(__float_as_uint(q) >> 23) - 127, 126);
  byte = (unsigned)(127 - e);
  return __uint_as_float((unsigned)(e + 127) << 23);
}

// amax bits of 8 bf16 held in 4 words, then the 8 scaled, clamped and converted bytes
__device__ __forceinline__ unsigned amax8(const unsigned (&w)[4]) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m = max(m, (w[j] << 16) & 0x7fffffffu);
    m = max(m, w[j] & 0x7fff0000u);
  }
  return m;
}

template <int FMT>
__device__ __forceinline__ uint2 quant8(const unsigned (&w)[4], float s) {
  const float lim = fmax_of(FMT);
  float f[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = fminf(fmaxf(__uint_as_float(w[j] << 16) * s, -lim), lim);
    f[2 * j + 1] = fminf(fmaxf(__uint_as_float(w[j] & 0xffff0000u) * s, -lim), lim);
  }
  return make_uint2(cvt4<FMT>(f[0], f[1], f[2], f[3]), cvt4<FMT>(f[4], f[5], f[6], f[7]));
}

// The two scale bytes a 64-wide tile owns of word [t >> 1][line] (t = the tile's index along the quantised axis,
// `lines` = the other extent): bytes 2 (t & 1) and + 1.  The last tile of an even t also owns the word's other half,
// which no tile covers: blocks at k >= K, byte 127.
__device__ __forceinline__ void store_scales(uint8_t* s, int t, size_t lines, size_t line, unsigned b0, unsigned b1,
                                             bool last) {
  uint8_t* w = s + (((size_t)(t >> 1) * lines + line) << 2);
  *(unsigned short*)(w + 2 * (t & 1)) = (unsigned short)(b0 | (b1 << 8));
  if (last && !(t & 1)) *(unsigned short*)(w + 2) = (unsigned short)0x7f7f;
}

template <int FMT>
__global__ void __launch_bounds__(256) mxfp8_cast_kernel(const __bf16* __restrict__ x, uint8_t* __restrict__ q,
                                                         uint8_t* __restrict__ sq, uint8_t* __restrict__ qt,
                                                         uint8_t* __restrict__ sqt, int R, int C) {
  __shared__ __attribute__((aligned(16))) char tile[64 * 128];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int r0 = by * 64, c0 = bx * 64;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int rl = 32 * p + (tid >> 3), c8 = tid & 7;
    const int r = r0 + rl, c = c0 + 8 * c8;
    const bool ok = r < R && c < C;  // R, C multiples of 32: a 32-block is inside or outside as a whole
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *(const uint4*)(x + (size_t)r * C + c);
    *(uint4*)(tile + rl * 128 + ((c8 ^ (rl >> 3)) << 4)) = v;
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned byte;
    const float s = block_scale<FMT>(quad_max(amax8(w)), byte);  // zeros outside: byte 127
    const uint2 o = quant8<FMT>(w, s);
    if (ok) *(uint2*)(q + (size_t)r * C + c) = o;
    const unsigned b1 = (unsigned)__shfl_down((int)byte, 4);
    if (ok && c8 == 0) store_scales(sq, bx, (size_t)R, (size_t)r, byte, b1, c0 + 64 >= C);
  }
  __syncthreads();
  const int g = tid & 7;  // row group: rows 8 g .. 8 g + 7
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int cl = 32 * i + (tid >> 3);
    const int c = c0 + cl;
    const bool ok = c < C && r0 + 8 * g < R;
    const char* src = tile + (((cl >> 3) ^ g) << 4) + 2 * (cl & 7);
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = (unsigned)*(const unsigned short*)(src + (8 * g + 2 * j) * 128) |
             ((unsigned)*(const unsigned short*)(src + (8 * g + 2 * j + 1) * 128) << 16);
    unsigned byte;
    const float s = block_scale<FMT>(quad_max(amax8(w)), byte);
    const uint2 o = quant8<FMT>(w, s);
    if (ok) *(uint2*)(qt + (size_t)c * R + r0 + 8 * g) = o;
    const unsigned b1 = (unsigned)__shfl_down((int)byte, 4);
    if (ok && g == 0) store_scales(sqt, by, (size_t)C, (size_t)c, byte, b1, r0 + 64 >= R);
  }
}

// ------------------------------------------------------------------------------------------------ the GEMM
constexpr int BM = 128, BN = 128, BK = 128, NTH = 256, NW = 4;
constexpr int IMG = 16384;            // one operand's K-tile: 128 rows x 128 B
constexpr int STAGE = 2 * IMG;        // [A | B]
constexpr int LDS_BYTES = 2 * STAGE;  // 64 KiB: two blocks per CU
constexpr int PIECES = IMG / 1024 / NW;  // 1 KiB DMA pieces per wave per image

// An offset no resource of this file contains: every extent is below 2^31 bytes.
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

struct MxArgs {
  const uint8_t* A;    // [M][lda] bytes, K-major
  const uint8_t* B;    // [N][ldb] bytes, K-major, E4M3
  const uint32_t* sA;  // [ceil(K / 128)][M] scale words
  const uint32_t* sB;  // [ceil(K / 128)][N]
  void* C;             // bf16 [M][ldc], or fp32 slabs [splits][M][N] when K is split
  void* C2;            // bf16 [M][ldc]: gelu_tanh of the stored C, or null
  int M, N, K, lda, ldb, ldc;
  int kt_per_split;    // K-tiles per blockIdx.y
  float alpha;
  const float* bias;   // fp32 [N] or null
  int group;           // M-tiles per tile group (tile_of)
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

// One operand's scale words for this lane: rows c0 + 16 t + fr, t = 0..3, of the [nkt][R] array.  The resource ends
// at the array's true last byte; a row past the edge keeps an offset >= 2^31 at every K-tile (the array is below 2^31
// bytes, checked by the host), so it reads 0.
struct Scales {
  __amdgpu_buffer_rsrc_t r;
  uint32_t off[4];
  uint32_t per_kt;  // bytes from one K-tile's words to the next

  __device__ __forceinline__ Scales(const uint32_t* S, int R, int nkt, int c0, int fr) {
    r = rsrc(S, (uint32_t)nkt * (uint32_t)R * 4u);
    per_kt = (uint32_t)R * 4u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = c0 + 16 * t + fr;
      off[t] = row < R ? (uint32_t)row * 4u : OOB;
    }
  }

  // the words of absolute K-tile kt
  __device__ __forceinline__ void load(int kt, uint32_t (&w)[4]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      w[t] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, (int)(off[t] + (uint32_t)kt * per_kt), 0, 0);
  }
};

__device__ __forceinline__ i32x8 ld_frag(const char* img, int o0, int o1) {
  const i32x4 lo = *(const i32x4*)(img + o0), hi = *(const i32x4*)(img + o1);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// acc += the wave's 64 x 64 part of the tile at (m0, n0) over K-tiles [kt0, kt0 + nk)
template <int AFMT>
__device__ __forceinline__ void mx_tile(const MxArgs& p, int m0, int n0, int kt0, int nk, f32x4 (&acc)[4][4],
                                        char* smem, int wave, int lane, int wm, int wn) {
  const Stager sa(p.A, p.lda, p.M, p.K, m0, kt0 * BK, wave, lane);
  const Stager sb(p.B, p.ldb, p.N, p.K, n0, kt0 * BK, wave, lane);

  // kswz(c0 + fr) = kswz(fr) for a 16-aligned c0: the two chunk offsets depend on the lane only; tile t adds 2048 B
  const int fr = lane & 15, fq = lane >> 4;
  // registers 0-3: k = 16 fq .. + 15 (chunk fq), registers 4-7: k = 64 + 16 fq .. + 15 (chunk 4 + fq)
  const int o0 = fr * 128 + ((fq ^ kswz(fr)) << 4), o1 = fr * 128 + (((4 + fq) ^ kswz(fr)) << 4);
  const int abase = wm * 64 * 128, bbase = wn * 64 * 128;

  const int nkt = (p.K + BK - 1) / BK;
  const Scales xa(p.sA, p.M, nkt, m0 + wm * 64, fr);
  const Scales xb(p.sB, p.N, nkt, n0 + wn * 64, fr);
  const int sh = 8 * fq;  // this lane supplies the scale of MX block fq of the K-tile: byte fq of the word
  uint32_t wa[4], wb[4];  // the words of the tile about to be multiplied

  auto step = [&](auto cb, int kt) {
    constexpr int CB = decltype(cb)::value;
    const char* ia = smem + CB * STAGE + abase;
    const char* ib = smem + CB * STAGE + IMG + bbase;
    // this wave's DMAs of tile kt have landed and its earlier LDS reads are done; after the barrier, everyone's
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    i32x8 fa[4], fb[4];
    int ca[4], cb_[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fa[t] = ld_frag(ia + t * 2048, o0, o1);
      fb[t] = ld_frag(ib + t * 2048, o0, o1);
      ca[t] = (int)(wa[t] >> sh);
      cb_[t] = (int)(wb[t] >> sh);
    }
    if (kt + 1 < nk) {  // the other stage: last read in step kt - 1, before the barrier above
      sa.issue(kt + 1, smem + (1 - CB) * STAGE, wave);
      sb.issue(kt + 1, smem + (1 - CB) * STAGE + IMG, wave);
      xa.load(kt0 + kt + 1, wa);
      xb.load(kt0 + kt + 1, wb);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)  // byte 0 (op_sel 0) of lane fr + 16 b's word scales block b of row fr
        acc[nt][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[nt], fa[mt], acc[nt][mt], E4M3, AFMT, 0,
                                                                       cb_[nt], 0, ca[mt]);
  };

  sa.issue(0, smem, wave);
  sb.issue(0, smem + IMG, wave);
  xa.load(kt0, wa);
  xb.load(kt0, wb);
  for (int kt = 0; kt < nk; kt += 2) {
    step(IC<0>{}, kt);
    if (kt + 1 < nk) step(IC<1>{}, kt + 1);
  }
}

// ACC: C += alpha * AB (bf16 read-modify-write); SLAB: write fp32 raw sums (split K)
template <int AFMT, bool ACC, bool SLAB>
__global__ void __launch_bounds__(NTH, 2) gemm_mxfp8_kernel(MxArgs p) {
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
  mx_tile<AFMT>(p, m0, n0, kt0, nk, acc, smem, wave, lane, wm, wn);

  // acc[nt][mt] is a 16 x 16 tile D[n][m]: m = lane & 15, n = 4 (lane >> 4) + j, j = 0..3
  const float s = SLAB ? 1.f : p.alpha;
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

// C (bf16, ldc) = alpha * sum over splits (in split order) of the fp32 slabs (+ bias) (+ C when accumulating)
// (C2: gelu_tanh of the stored C); 8 elements per thread (N is a multiple of 8: a thread's 8 stay in one row)
template <bool ACC>
__global__ void __launch_bounds__(256) gemm_mxfp8_reduce(const float* __restrict__ ws, __bf16* __restrict__ C,
                                                         __bf16* __restrict__ C2, int M, int N, int ldc, int splits,
                                                         float alpha, const float* __restrict__ bias) {
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
  s[0] *= alpha;
  s[1] *= alpha;
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
int launch(const MxArgs& a, int splits, hipStream_t st) {
  auto k = gemm_mxfp8_kernel<AFMT, ACC, SLAB>;
  static const int attr =
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) == hipSuccess ? 0 : -4;
  if (attr) return attr;
  const dim3 grid(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), splits);
  hipLaunchKernelGGL(k, grid, dim3(NTH), LDS_BYTES, st, a);
  return 0;
}

template <int AFMT>
int dispatch(const MxArgs& a, int splits, int accumulate, hipStream_t st) {
  if (splits > 1) return launch<AFMT, false, true>(a, splits, st);
  return accumulate ? launch<AFMT, true, false>(a, 1, st) : launch<AFMT, false, false>(a, 1, st);
}

constexpr int kSplitTarget = 512;  // blocks the split-K planner aims for: two per CU of a 256-CU chip
constexpr int kGroup = 4;

bool shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && M % 16 == 0 && N % 16 == 0 && K % 32 == 0; }

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
PLX_API int plx_gemm_mxfp8_splits(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return 0;
  const int kps = plan_kt_per_split(M, N, K);
  return ((K + BK - 1) / BK + kps - 1) / kps;
}

// fp32 workspace floats the launch needs (0 when K is not split, -1 for a shape the kernel does not take)
PLX_API long long plx_gemm_mxfp8_ws(int M, int N, int K) {
  if (!shape_ok(M, N, K)) return -1;
  const int s = plx_gemm_mxfp8_splits(M, N, K);
  return s > 1 ? (long long)s * M * N : 0;
}

PLX_API int plx_gemm_mxfp8_tile() { return BM; }

// q [R][C] with scale words sq [ceil(C / 128)][R] and qt [C][R] with sqt [ceil(R / 128)][C] (FP8 bytes of format fmt,
// E8M0 scale bytes) from x [R][C] (bf16); R, C multiples of 32
PLX_API int plx_mxfp8_cast(const void* x, void* q, void* sq, void* qt, void* sqt, int R, int C, int fmt,
                           void* stream) {
  if (R <= 0 || C <= 0 || R % 32 || C % 32 || (fmt != E4M3 && fmt != E5M2)) return -1;
  if ((uintptr_t)x % 16 || (uintptr_t)q % 8 || (uintptr_t)qt % 8 || !sq || !sqt || (uintptr_t)sq % 4 ||
      (uintptr_t)sqt % 4)
    return -1;
  const dim3 grid((C + 63) / 64, (R + 63) / 64);
  if (grid.y > 65535) return -2;
  if (fmt == E5M2)
    hipLaunchKernelGGL(mxfp8_cast_kernel<E5M2>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, (uint8_t*)q,
                       (uint8_t*)sq, (uint8_t*)qt, (uint8_t*)sqt, R, C);
  else
    hipLaunchKernelGGL(mxfp8_cast_kernel<E4M3>, grid, dim3(256), 0, (hipStream_t)stream, (const __bf16*)x, (uint8_t*)q,
                       (uint8_t*)sq, (uint8_t*)qt, (uint8_t*)sqt, R, C);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// C[M][N] (bf16, ldc) = alpha * (A 2^(sA - 127)) . (B 2^(sB - 127))^T (+ bias[n]) (+ C when accumulate); A [M][lda]
// bytes of format a_fmt with scale words sA [ceil(K / 128)][M], B [N][ldb] E4M3 bytes with sB [ceil(K / 128)][N];
// M, N multiples of 16, K a multiple of 32.  bias: fp32 [N], 16-byte aligned, or null (not combined with accumulate).
// gelu_out: bf16 laid out like C receiving gelu_tanh(C), or null (not with accumulate).
// ws: plx_gemm_mxfp8_ws(M, N, K) floats, 16-byte aligned (may be null when that is 0).
// Returns 0, or < 0 on a shape / layout the kernel does not take (nothing launched).
PLX_API int plx_gemm_mxfp8(const void* A, const void* sA, const void* B, const void* sB, void* C, void* ws, int M, int N,
                           int K, int lda, int ldb, int ldc, int a_fmt, float alpha, int accumulate, const float* bias,
                           void* gelu_out, void* stream) {
  if (!shape_ok(M, N, K) || (a_fmt != E4M3 && a_fmt != E5M2) || !sA || !sB) return -1;
  if ((uintptr_t)sA % 4 || (uintptr_t)sB % 4) return -1;
  if (bias != nullptr && (accumulate || (uintptr_t)bias % 16)) return -1;
  if (gelu_out != nullptr && (accumulate || (uintptr_t)gelu_out % 16)) return -1;
  if (lda % 16 || ldb % 16 || ldc % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)C % 16) return -1;
  if (lda < K || ldb < K || ldc < N) return -1;
  // the largest byte offset a block forms relative to its tile origin, tails included (it must stay below 2^31)
  if ((long long)BM * lda + K + BK >= 0x7ffffff0LL || (long long)BN * ldb + K + BK >= 0x7ffffff0LL) return -2;
  const long long nkt = (K + BK - 1) / BK;
  if (nkt * M * 4 >= 0x7ffffff0LL || nkt * N * 4 >= 0x7ffffff0LL) return -2;  // the scale arrays, in bytes
  const int kps = plan_kt_per_split(M, N, K);
  const int splits = ((K + BK - 1) / BK + kps - 1) / kps;
  if (splits > 1 && (!ws || (uintptr_t)ws % 16)) return -5;
  MxArgs a{(const uint8_t*)A, (const uint8_t*)B, (const uint32_t*)sA, (const uint32_t*)sB, splits > 1 ? ws : C,
           splits > 1 ? nullptr : gelu_out, M, N, K, lda, ldb, ldc, kps, alpha, bias, kGroup};
  hipStream_t st = (hipStream_t)stream;
  const int rc = a_fmt == E5M2 ? dispatch<E5M2>(a, splits, accumulate, st) : dispatch<E4M3>(a, splits, accumulate, st);
  if (rc) return rc;
  if (splits > 1) {
    const size_t total8 = (size_t)M * N / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256));
    if (accumulate)
      hipLaunchKernelGGL(gemm_mxfp8_reduce<true>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C,
                         (__bf16*)nullptr, M, N, ldc, splits, alpha, (const float*)nullptr);
    else
      hipLaunchKernelGGL(gemm_mxfp8_reduce<false>, grid, dim3(256), 0, st, (const float*)ws, (__bf16*)C,
                         (__bf16*)gelu_out, M, N, ldc, splits, alpha, bias);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
