// CRC-32 (zlib's: reflected polynomial 0xEDB88320, seed and result complemented outside the register) of many rows of bytes
// that are in device memory, their lengths too: the checksum of PNG's chunks (png.hip: sp_png_wrap), and what gzip and zip
// would need.  include/svdpipe.h fixes the rules.
//
// A row is cut into pieces of PIECE = 64 bytes from its first byte on, and a workgroup of 256 takes SPAN = 256 pieces
// (16 KiB).  The register of a piece is linear in its start value and its bytes, so the piece that holds byte 0 starts from
// ~seed and every other piece from 0, a register with k bytes behind it is multiplied by x^(8k) mod P in GF(2), and the XOR of
// all of them is the register of the whole row (zlib's crc32_combine, on registers and not on finished checksums).
//
//   crc32_span_kernel : a workgroup per (row, span).  The span comes into LDS in whole words by coalesced loads (aligned
//                       dwords put together by v_alignbyte where the row's address is not a multiple of 4; bytes at the two
//                       ends of the row, so that nothing outside row[0 .. len) is read), a piece at a stride of 17 words: the
//                       lanes of a wave then read 32 different banks at every step.  A thread walks its piece table-free: the
//                       word is XORed in and the register shifted 32 times (3 VALU operations per bit and no table whose
//                       lookups would collide in LDS; 24 operations per byte are some 10 us of the chip for a video's 17 MB).
//                       Its register is then multiplied up to the span's end (one multiplication of 32 shift-and-xor steps
//                       per set bit of the byte count, by the constants x^(2^k) mod P) and the workgroup's XOR goes to ws.
//   crc32_fold_kernel : a workgroup per row multiplies every span's register up to the row's end, XORs them and complements.
// Spans behind a row's length leave at once: the grid is sized by the pitch, which the host knows, and not by the lengths,
// which it does not.
#include "codec_common.h"

namespace {

constexpr u32 POLY = 0xEDB88320u;
constexpr int PIECE = 64, PIECE_WORDS = PIECE / 4, PIECE_STRIDE = PIECE_WORDS + 1;
constexpr int SPAN = 256 * PIECE;

// a(x) * b(x) mod P, bit 31 the coefficient of x^0 (zlib's multmodp without its early exit)
constexpr u32 mulmod_host(u32 a, u32 b) {
  u32 p = 0;
  for (int i = 31; i >= 0; --i) {
    if ((a >> i) & 1u) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? POLY : 0u);
  }
  return p;
}
struct Powers {
  u32 v[32];                             // x^(2^k) mod P
};
constexpr Powers make_powers() {
  Powers t{};
  u32 p = 1u << 30;                      // x^1
  t.v[0] = p;
  for (int k = 1; k < 32; ++k) {
    p = mulmod_host(p, p);
    t.v[k] = p;
  }
  return t;
}
__constant__ Powers X2N = make_powers();

__device__ __forceinline__ u32 mulmod(u32 a, u32 b) {
  u32 p = 0;
#pragma unroll
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
  }
  return p;
}

// the register after `bytes` more zero bytes: reg * x^(8 bytes) mod P.  x has an order that divides 2^32 - 1, so x^(2^32) is x
// again and the table is indexed mod 32 (zlib's x2nmodp).
__device__ __forceinline__ u32 advance(u32 reg, u32 bytes) {
  for (int k = 3; bytes; bytes >>= 1, ++k)
    if (bytes & 1u) reg = mulmod(X2N.v[k & 31], reg);
  return reg;
}

__device__ __forceinline__ u32 shift_bits(u32 reg, int bits) {
  for (int i = 0; i < bits; ++i) reg = (reg >> 1) ^ (POLY & (0u - (reg & 1u)));
  return reg;
}

__device__ __forceinline__ int clamp_len(int len, int64_t pitch) { return len < 0 ? 0 : ((int64_t)len > pitch ? (int)pitch : len); }

// grid: rows * spans workgroups of 256, spans = ceil(pitch / SPAN)
__global__ __launch_bounds__(256) void crc32_span_kernel(const u8 *__restrict__ data, int64_t pitch, const int *__restrict__ lens,
                                                         const u32 *__restrict__ seed, int spans, u32 *__restrict__ partial) {
  __shared__ u32 words[256 * PIECE_STRIDE];
  __shared__ u32 wave_reg[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t bid = blockIdx.x;
  const int sp = (int)(bid % spans);
  const int64_t row = bid / spans;
  const int len = clamp_len(lens[row], pitch);
  const int64_t b0 = (int64_t)sp * SPAN;
  if (b0 >= len) return;                                     // (the whole workgroup)
  const u8 *src = data + row * pitch;
  const int span = (int)min((int64_t)SPAN, len - b0);
  for (int j = tid; 4 * j < span; j += 256) words[j + j / PIECE_WORDS] = load_bytes4(src, b0 + 4 * j, len);
  __syncthreads();
  const int start = tid * PIECE, mine = min(PIECE, span - start);   // (mine <= 0: no byte of the span is this thread's)
  u32 reg = 0;
  if (mine > 0) {
    if (b0 == 0 && tid == 0) reg = ~(seed ? seed[row] : 0u);
    const u32 *wp = words + tid * PIECE_STRIDE;
    const int full = mine >> 2, rest = mine & 3;
    for (int k = 0; k < full; ++k) reg = shift_bits(reg ^ wp[k], 32);
    if (rest) reg = shift_bits(reg ^ (wp[full] & ((1u << (8 * rest)) - 1u)), 8 * rest);
    reg = advance(reg, (u32)(span - start - mine));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) reg ^= __shfl_xor(reg, o, 64);
  if (lane == 0) wave_reg[wv] = reg;
  __syncthreads();
  if (tid == 0) partial[bid] = wave_reg[0] ^ wave_reg[1] ^ wave_reg[2] ^ wave_reg[3];
}

// grid: one workgroup of 256 per row
__global__ __launch_bounds__(256) void crc32_fold_kernel(const u32 *__restrict__ partial, int64_t pitch, const int *__restrict__ lens,
                                                         const u32 *__restrict__ seed, int spans, u32 *__restrict__ crc) {
  __shared__ u32 wave_reg[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = blockIdx.x;
  const int len = clamp_len(lens[row], pitch);
  const int used = (int)(((int64_t)len + SPAN - 1) / SPAN);
  u32 reg = 0;
  for (int j = tid; j < used; j += 256) {
    const int64_t end = min((int64_t)len, ((int64_t)j + 1) * SPAN);
    reg ^= advance(partial[row * spans + j], (u32)(len - end));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) reg ^= __shfl_xor(reg, o, 64);
  if (lane == 0) wave_reg[wv] = reg;
  __syncthreads();
  if (tid == 0) crc[row] = len == 0 ? (seed ? seed[row] : 0u) : ~(wave_reg[0] ^ wave_reg[1] ^ wave_reg[2] ^ wave_reg[3]);
}

}  // namespace

extern "C" size_t sp_crc32_ws_bytes(int n, size_t pitch) {
  if (n <= 0 || pitch == 0 || pitch > (size_t)0x7fffffff) return 0;
  return sizeof(u32) * (size_t)n * ((pitch + SPAN - 1) / SPAN);
}

// the two launches, for sp_crc32_rows and for sp_png_wrap; the caller has checked the arguments
void sp_crc32_launch(const void *data, size_t pitch, const void *lens, const void *seed, int n, void *crc, void *ws, hipStream_t s) {
  const int spans = (int)((pitch + SPAN - 1) / SPAN);
  hipLaunchKernelGGL(crc32_span_kernel, dim3((unsigned)((int64_t)n * spans)), dim3(256), 0, s, (const u8 *)data, (int64_t)pitch,
                     (const int *)lens, (const u32 *)seed, spans, (u32 *)ws);
  hipLaunchKernelGGL(crc32_fold_kernel, dim3((unsigned)n), dim3(256), 0, s, (const u32 *)ws, (int64_t)pitch, (const int *)lens,
                     (const u32 *)seed, spans, (u32 *)crc);
}

extern "C" int sp_crc32_rows(const void *data, size_t pitch, const void *lens, const void *seed, int n, void *crc, void *ws,
                             size_t ws_bytes, void *stream) {
  SP_REQUIRE(data && lens && crc && ws, "sp_crc32_rows: null pointer");
  SP_REQUIRE(n > 0 && pitch > 0 && pitch <= (size_t)0x7fffffff, "sp_crc32_rows: n must be positive and pitch in 1..2^31-1 (n=%d, pitch=%zu)",
             n, pitch);
  const size_t need = sp_crc32_ws_bytes(n, pitch);
  SP_REQUIRE(ws_bytes >= need, "sp_crc32_rows: ws holds %zu bytes, needs %zu (sp_crc32_ws_bytes)", ws_bytes, need);
  SP_REQUIRE((uintptr_t)ws % 4 == 0 && (uintptr_t)lens % 4 == 0 && (uintptr_t)crc % 4 == 0 && (uintptr_t)seed % 4 == 0,
             "sp_crc32_rows: lens, seed, crc and ws must be 4-byte aligned");
  SP_REQUIRE(need / sizeof(u32) <= (size_t)0x7fffffff, "sp_crc32_rows: too many spans (%zu)", need / sizeof(u32));
  SP_CLEAR_STALE_ERROR();
  sp_crc32_launch(data, pitch, lens, seed, n, crc, ws, (hipStream_t)stream);
  SP_CHECK_LAUNCH("sp_crc32_rows");
  return SP_OK;
}
