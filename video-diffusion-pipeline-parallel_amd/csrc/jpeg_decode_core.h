// The parts of the baseline JPEG decoder (jpeg_decode.hip) that a host program can run too: the plan a parsed header becomes
// (sizes, table selectors, derived Huffman tables, the layout of the scratch buffer), one lane's decode step, the guarded
// coefficient store and the integer pixel arithmetic.  Plain inline functions behind JD_HD, so that the kernels and tools/jpeg_decode_hostcheck.cpp (built with
// the host sanitizers) execute the same text.  include/svdpipe.h fixes the rules.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

#define JD_MAGIC 0x4a444331            /* "JDC1" */
#define JD_FIELDS 17                   /* w h ncomp hs vs restart seg_len subseq_bits tq[3] td[3] ta[3] */
#define JD_MAX_SEGMENT (1 << 28)       /* bytes: every bit position stays below 2^31 */

// words of the status block at the front of the scratch buffer (int32)
enum { JD_M_ERROR = 0, JD_M_FIXED = 1, JD_M_PASSES = 2, JD_M_CLEAN = 3, JD_M_MARKERS = 4, JD_M_SUBS = 5, JD_M_LONGEST = 6,
       JD_M_CHANGED = 7 /* 3 words */, JD_M_COEF_DONE = 10, JD_M_WORDS = 64 };
// bits of the error word
enum { JD_E_MARKER = 1, JD_E_RST_ORDER = 2, JD_E_RST_COUNT = 4, JD_E_CODE = 8, JD_E_BLOCKS = 16 };

enum { JD_CONT = 0, JD_STOP = 1, JD_ERR = 2 };      /* of a step; a lane's run returns STOP and ERR as bits */

typedef struct JdParams {
  int32_t magic;
  int32_t w, h, ncomp, hs, vs;         // hs, vs: luminance sampling (1 or 2); chrominance is 1 x 1
  int32_t mcu_cols, mcu_rows, bpm;     // bpm: blocks per MCU (1, 3, 4 or 6)
  int32_t restart;                     // MCUs per interval (all of them in a file without DRI)
  int32_t n_iv, total_mcus;
  int32_t seg_len, subseq_bits, max_sub;
  int32_t blk_comp[6], blk_dc[6], blk_ac[6];   // per block of the MCU: component, Huffman table (0, 1: DC; 2, 3: AC)
  int32_t comp_tq[3];
} JdParams;

typedef struct JdHuff {
  uint16_t look[512];                  // 9 bits ahead: length << 8 | symbol, 0 where the code is longer
  int32_t maxcode[17];                 // largest code of each length, -1 where there is none
  int32_t valoff[17];                  // index of the first symbol of that length minus its first code
  int32_t nvals;
  uint8_t vals[256];
} JdHuff;

typedef struct JdTables {
  uint8_t quant[4][64];                // natural (row-major) order
  JdHuff huff[4];
} JdTables;

typedef struct JdPlan {
  JdParams p;
  JdTables t;
} JdPlan;

// a lane's record of one pass: where it started, where it stopped, and the blocks it completed in between
typedef struct JdRec {
  uint32_t in_pos, in_st, out_pos, out_st, nblk, err;
} JdRec;

typedef struct JdLane {
  uint32_t pos;                        // absolute bit position in the clean stream
  int32_t blk, zz;                     // block of the MCU, zigzag index of the next coefficient (0: the DC symbol is next)
  uint32_t nblk;                       // blocks completed since the lane started
} JdLane;

// byte offsets into the scratch buffer, all multiples of 256
typedef struct JdLayout {
  size_t meta, blk_keep, blk_mark, clean, iv_start, sub_first, rec0, rec1, lane_first, lane_part, dc_carry, planes, total;
  size_t clean_cap;                    // bytes of the clean stream's slot (seg_len up to a word, plus one word)
  int32_t byte_blocks;                 // workgroups of the byte passes (JD_BYTES_PER_BLOCK each)
  int32_t lane_parts;                  // groups of JD_LANES_PER_PART lanes
  int32_t dc_chunks;                   // groups of 256 MCUs
  int32_t luma_w, luma_h, chroma_w, chroma_h;   // the planes the inverse DCT writes (whole MCUs)
} JdLayout;

#define JD_BYTES_PER_BLOCK 4096
#define JD_LANES_PER_PART 2048

JD_HD size_t jd_up256(size_t v) { return (v + 255) & ~(size_t)255; }

JD_HD void jd_layout(const JdParams *p, JdLayout *L) {
  size_t at = 0;
  L->byte_blocks = (p->seg_len + JD_BYTES_PER_BLOCK - 1) / JD_BYTES_PER_BLOCK;
  L->lane_parts = (p->max_sub + JD_LANES_PER_PART - 1) / JD_LANES_PER_PART;
  L->dc_chunks = (p->total_mcus + 255) / 256;
  L->luma_w = p->mcu_cols * 8 * p->hs, L->luma_h = p->mcu_rows * 8 * p->vs;
  L->chroma_w = p->ncomp == 3 ? p->mcu_cols * 8 : 0, L->chroma_h = p->ncomp == 3 ? p->mcu_rows * 8 : 0;
  L->clean_cap = (((size_t)p->seg_len + 3) & ~(size_t)3) + 4;
  L->meta = at, at += jd_up256(JD_M_WORDS * 4);
  L->blk_keep = at, at += jd_up256((size_t)(L->byte_blocks + 1) * 4);
  L->blk_mark = at, at += jd_up256((size_t)(L->byte_blocks + 1) * 4);
  L->clean = at, at += jd_up256(L->clean_cap);
  L->iv_start = at, at += jd_up256(((size_t)p->n_iv + 1) * 4);
  L->sub_first = at, at += jd_up256(((size_t)p->n_iv + 1) * 4);
  L->rec0 = at, at += jd_up256((size_t)p->max_sub * sizeof(JdRec));
  L->rec1 = at, at += jd_up256((size_t)p->max_sub * sizeof(JdRec));
  L->lane_first = at, at += jd_up256(((size_t)p->max_sub + 1) * 4);
  L->lane_part = at, at += jd_up256(((size_t)L->lane_parts + 1) * 4);
  L->dc_carry = at, at += jd_up256((size_t)L->dc_chunks * 16);
  L->planes = at, at += jd_up256((size_t)L->luma_w * L->luma_h + 2 * (size_t)L->chroma_w * L->chroma_h);
  L->total = at;
}

// MCUs of interval k
JD_HD int32_t jd_interval_mcus(const JdParams *p, int32_t k) {
  const int64_t left = (int64_t)p->total_mcus - (int64_t)k * p->restart;
  return (int32_t)(left < p->restart ? left : p->restart);
}

// Host.  bits16 / vals of a DHT segment -> the derived table.  0, or -1 for a specification no canonical code has: more than
// 256 symbols, more codes of a length than that length has, or the all-ones code assigned (T.81 C.2 forbids it, and the
// padding 1-bits at an interval's end rely on that).
inline int jd_build_huff(const uint8_t *bits16, const uint8_t *vals, JdHuff *h) {
  int total = 0;
  for (int i = 0; i < 16; ++i) total += bits16[i];
  if (total > 256) return -1;
  for (int i = 0; i < 512; ++i) h->look[i] = 0;
  for (int i = 0; i < 256; ++i) h->vals[i] = i < total ? vals[i] : 0;
  h->nvals = total;
  h->maxcode[0] = -1, h->valoff[0] = 0;
  int32_t code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits16[l - 1];
    if (code + n > (1 << l) - 1 + (n == 0)) return -1;          // (the last code of the length would be all ones, or past it)
    h->valoff[l] = k - code;
    for (int j = 0; j < n; ++j, ++code, ++k)
      if (l <= 9)
        for (int f = 0; f < (1 << (9 - l)); ++f) h->look[(code << (9 - l)) + f] = (uint16_t)((l << 8) | vals[k]);
    h->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  return 0;
}

// Host.  The 17 header fields plus the tables of the file -> a plan.  0, or -1 with a reason for fields the decoder refuses.
// `have_q` / `have_h`: bit i set where table i was defined (Huffman: 0, 1 DC; 2, 3 AC).
inline int jd_make_plan(const int32_t *f, const uint8_t *quant4x64, int have_q, const uint8_t *bits4x16, const uint8_t *vals4x256,
                        int have_h, JdPlan *pl, const char **why) {
  JdParams *p = &pl->p;
  const int32_t w = f[0], h = f[1], ncomp = f[2], hs = f[3], vs = f[4], restart = f[5], seg_len = f[6], subseq = f[7];
  *why = "size must be 1..65535 on a side";
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return -1;
  *why = "one component, or three with luminance sampled 1x1, 2x1 or 2x2";
  if (!(ncomp == 1 || ncomp == 3) || !(hs == 1 || hs == 2) || !(vs == 1 || vs == 2) || (hs == 1 && vs == 2)) return -1;
  if (ncomp == 1 && (hs != 1 || vs != 1)) return -1;
  *why = "restart interval must be 0..65535";
  if (restart < 0 || restart > 65535) return -1;
  *why = "the entropy-coded segment must hold 1..2^28-1 bytes";
  if (seg_len < 1 || seg_len >= JD_MAX_SEGMENT) return -1;
  *why = "subseq_bits must be a multiple of 32, at least 32 and at most 2^20";
  if (subseq < 32 || subseq % 32 || subseq > (1 << 20)) return -1;
  p->magic = JD_MAGIC;
  p->w = w, p->h = h, p->ncomp = ncomp, p->hs = hs, p->vs = vs;
  p->mcu_cols = (w + 8 * hs - 1) / (8 * hs), p->mcu_rows = (h + 8 * vs - 1) / (8 * vs);
  p->bpm = ncomp == 1 ? 1 : hs * vs + 2;
  p->total_mcus = p->mcu_cols * p->mcu_rows;
  p->restart = restart ? (restart < p->total_mcus ? restart : p->total_mcus) : p->total_mcus;
  p->n_iv = (p->total_mcus + p->restart - 1) / p->restart;
  p->seg_len = seg_len, p->subseq_bits = subseq;
  p->max_sub = (int32_t)(((int64_t)seg_len * 8 + subseq - 1) / subseq) + p->n_iv + 1;
  *why = "a table selector without its table";
  for (int b = 0; b < 6; ++b) {
    const int c = ncomp == 1 ? 0 : (b < hs * vs ? 0 : (b - hs * vs + 1 > 2 ? 2 : b - hs * vs + 1));
    const int32_t td = f[11 + c], ta = f[14 + c];
    if (td < 0 || td > 1 || ta < 0 || ta > 1) return -1;
    if (!((have_h >> td) & 1) || !((have_h >> (2 + ta)) & 1)) return -1;
    p->blk_comp[b] = c, p->blk_dc[b] = td, p->blk_ac[b] = 2 + ta;
  }
  for (int c = 0; c < 3; ++c) {
    const int32_t tq = f[8 + (c < ncomp ? c : 0)];
    if (tq < 0 || tq > 3 || !((have_q >> tq) & 1)) return -1;
    p->comp_tq[c] = tq;
  }
  for (int t = 0; t < 4; ++t)
    for (int i = 0; i < 64; ++i) pl->t.quant[t][i] = ((have_q >> t) & 1) ? quant4x64[t * 64 + i] : 1;
  *why = "a Huffman table specification that no canonical code has";
  for (int t = 0; t < 4; ++t) {
    static const uint8_t none[16] = {0};
    if (jd_build_huff(((have_h >> t) & 1) ? bits4x16 + 16 * t : none, vals4x256 + 256 * t, &pl->t.huff[t]) != 0) return -1;
  }
  *why = "";
  return 0;
}

// Byte b of the segment between its neighbours (-1 behind the end): bit 0 kept, bit 1 an RSTn marker starts here, bit 2 an FF
// that neither stuffing nor RSTn follows.  The byte behind an FF (0x00, or RSTn's second byte) is dropped.
JD_HD int jd_classify(int prev, int b, int next) {
  if (b == 0xFF) return next == 0x00 ? 1 : (next >= 0xD0 && next <= 0xD7 ? 2 : 4);
  return prev == 0xFF ? 0 : 1;
}

JD_HD uint32_t jd_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// The 32 bits from bit `pos` of the clean stream (most significant first).  Reads words pos/32 and pos/32 + 1: the stream's
// slot holds one word more than its bytes (JdLayout::clean_cap), and callers only ask for a position below the stream's end.
JD_HD uint32_t jd_window(const uint32_t *words, uint32_t pos) {
  const uint32_t i = pos >> 5, s = pos & 31;
  const uint32_t a = jd_bswap(words[i]), b = jd_bswap(words[i + 1]);
  return s ? (a << s) | (b >> (32 - s)) : a;
}

// The symbol whose code starts the 16 bits `peek`, its length in *len; -1 for a code the table does not assign.
JD_HD int jd_symbol(const JdHuff *h, uint32_t peek, int *len) {
  const uint32_t e = h->look[peek >> 7];
  if (e) {
    *len = (int)(e >> 8);
    return (int)(e & 255);
  }
  for (int l = 10; l <= 16; ++l) {
    const int32_t code = (int32_t)(peek >> (16 - l));
    if (code <= h->maxcode[l]) {
      const int32_t idx = h->valoff[l] + code;
      if (idx < 0 || idx >= h->nvals) return -1;
      *len = l;
      return h->vals[idx];
    }
  }
  return -1;
}

// The guarded store: a coefficient goes to block `block` only below `block_end` (the end of the lane's interval) and only at
// a zigzag index 0..63; coef == null in the synchronisation passes, which only follow the state.
JD_HD void jd_store(int16_t *coef, uint32_t block, uint32_t block_end, int zz, int v) {
  if (coef && block < block_end && (unsigned)zz < 64u) coef[(size_t)block * 64 + (unsigned)zz] = (int16_t)v;
}

// One symbol of lane `ln` (ln->pos < end_bits): a DC difference where zz == 0, else run / size, ZRL or EOB.  JD_STOP, the lane
// unchanged, where the code plus its extra bits would pass the interval's end (`end_bits`; the all-ones padding completes no
// code).  JD_ERR for what no valid stream holds, after a step that keeps the lane going, because a lane that started at a
// wrong bit meets such things and has to find the true walk all the same: an unassigned code is passed over by one bit; a
// size above 11 (DC) / 10 (AC) is taken as it is; an index past 63, a ZRL past the block's end or an EOBn of progressive
// files ends the block.  `first_block` is the block the lane was in when it started.
JD_HD int jd_step(const uint32_t *words, uint32_t end_bits, const JdHuff *huff, const JdParams *p, JdLane *ln, int16_t *coef,
                  uint32_t first_block, uint32_t block_end) {
  const uint32_t pos = ln->pos;
  const uint32_t win = jd_window(words, pos);
  const int dc = ln->zz == 0;
  const JdHuff *h = huff + (dc ? p->blk_dc[ln->blk] : p->blk_ac[ln->blk]);
  int len = 0, flag = JD_CONT;
  const int sym = jd_symbol(h, win >> 16, &len);
  if (sym < 0) {
    if (end_bits - pos < 16) return JD_STOP;
    ln->pos = pos + 1;
    return JD_ERR;
  }
  const int size = dc ? sym : (sym & 15), run = dc ? 0 : (sym >> 4);
  if (pos + (uint32_t)(len + size) > end_bits) return JD_STOP;
  if (size > (dc ? 11 : 10)) flag = JD_ERR;
  int zz = ln->zz;
  if (!dc && size == 0) {
    if (run == 15) {
      zz += 16;
      if (zz > 64) zz = 64, flag = JD_ERR;
    } else {
      if (run != 0) flag = JD_ERR;
      zz = 64;
    }
  } else {
    zz += run;
    if (zz > 63) {
      zz = 64, flag = JD_ERR;
    } else {
      if (size) {
        const uint32_t bits = (win << len) >> (32 - size);
        const int v = bits < (1u << (size - 1)) ? (int)bits - (1 << size) + 1 : (int)bits;
        jd_store(coef, first_block + ln->nblk, block_end, zz, v);
      }
      ++zz;
    }
  }
  ln->pos = pos + (uint32_t)(len + size);
  if (zz == 64) {
    ln->zz = 0;
    ln->blk = ln->blk + 1 == p->bpm ? 0 : ln->blk + 1;
    ++ln->nblk;
  } else {
    ln->zz = zz;
  }
  return flag;
}

// A lane from its start until it has stepped past `sub_end` (<= end_bits) or has to stop: JD_STOP and JD_ERR as bits.
JD_HD int jd_lane_run(const uint32_t *words, uint32_t end_bits, uint32_t sub_end, const JdHuff *huff, const JdParams *p, JdLane *ln,
                      int16_t *coef, uint32_t first_block, uint32_t block_end) {
  int seen = 0;
  while (ln->pos < sub_end) {
    const int r = jd_step(words, end_bits, huff, p, ln, coef, first_block, block_end);
    seen |= r;
    if (r == JD_STOP) break;
  }
  return seen;
}

// Lane j of an interval whose bits are [bit0, end_bits), in pass `pass`: `prev` is lane j - 1's record of the pass before,
// `mine` this lane's.  Writes the record of this pass; 1 where its exit differs from `mine`'s.  `err` says that the walk met
// something invalid; it stays with the record and is not part of the state the next lane starts from, so at the fixed point,
// where every lane started from the true state, a set `err` is an error of the stream.
JD_HD int jd_lane_pass(const uint32_t *words, uint32_t bit0, uint32_t end_bits, uint32_t j, int pass, const JdHuff *huff,
                       const JdParams *p, const JdRec *prev, const JdRec *mine, JdRec *out) {
  uint32_t in_pos, in_st;
  if (j == 0) in_pos = bit0, in_st = 0;
  else if (pass == 0) in_pos = bit0 + j * (uint32_t)p->subseq_bits, in_st = 0;
  else in_pos = prev->out_pos, in_st = prev->out_st;
  JdRec r;
  r.in_pos = in_pos, r.in_st = in_st;
  if (pass > 0 && mine->in_pos == in_pos && mine->in_st == in_st) {
    r.out_pos = mine->out_pos, r.out_st = mine->out_st, r.nblk = mine->nblk, r.err = mine->err;   // the same start, the same walk
  } else {
    const uint64_t nominal = (uint64_t)bit0 + ((uint64_t)j + 1) * (uint32_t)p->subseq_bits;
    const uint32_t sub_end = nominal < end_bits ? (uint32_t)nominal : end_bits;
    JdLane ln;
    ln.pos = in_pos, ln.blk = (int32_t)(in_st >> 8), ln.zz = (int32_t)(in_st & 255), ln.nblk = 0;
    const int rc = jd_lane_run(words, end_bits, sub_end, huff, p, &ln, (int16_t *)0, 0, 0);
    r.out_pos = ln.pos, r.nblk = ln.nblk, r.err = (rc & JD_ERR) ? 1u : 0u;
    r.out_st = ((uint32_t)ln.blk << 8) | (uint32_t)ln.zz;
  }
  *out = r;
  return pass == 0 || r.out_pos != mine->out_pos || r.out_st != mine->out_st || r.nblk != mine->nblk || r.err != mine->err;
}

// ---------------------------------------------------------------------------------------------- pixels, in integers
// Dequantised coefficients (natural order, in[0..63]) -> 64 samples: libjpeg's accurate integer inverse DCT (jidctint: 13-bit
// constants, two extra bits kept after the column pass), the level shift and its range table (a clamp for values within
// +-512 of the range, which it wraps beyond).  Products and sums wrap in 32 bits.
JD_HD int32_t jd_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
JD_HD int32_t jd_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JD_HD int32_t jd_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
JD_HD int32_t jd_descale(int32_t x, int n) { return jd_add(x, 1 << (n - 1)) >> n; }

JD_HD void jd_idct_1d(const int32_t *v, int stride, int32_t *o, int ostride, int shift_even, int descale) {
  int32_t z2 = v[2 * stride], z3 = v[6 * stride];
  int32_t z1 = jd_mul(jd_add(z2, z3), 4433);
  int32_t tmp2 = jd_add(z1, jd_mul(z3, -15137)), tmp3 = jd_add(z1, jd_mul(z2, 6270));
  z2 = v[0], z3 = v[4 * stride];
  int32_t tmp0 = jd_mul(jd_add(z2, z3), 1 << shift_even), tmp1 = jd_mul(jd_sub(z2, z3), 1 << shift_even);
  const int32_t tmp10 = jd_add(tmp0, tmp3), tmp13 = jd_sub(tmp0, tmp3), tmp11 = jd_add(tmp1, tmp2), tmp12 = jd_sub(tmp1, tmp2);
  tmp0 = v[7 * stride], tmp1 = v[5 * stride], tmp2 = v[3 * stride], tmp3 = v[stride];
  z1 = jd_add(tmp0, tmp3), z2 = jd_add(tmp1, tmp2), z3 = jd_add(tmp0, tmp2);
  int32_t z4 = jd_add(tmp1, tmp3);
  const int32_t z5 = jd_mul(jd_add(z3, z4), 9633);
  tmp0 = jd_mul(tmp0, 2446), tmp1 = jd_mul(tmp1, 16819), tmp2 = jd_mul(tmp2, 25172), tmp3 = jd_mul(tmp3, 12299);
  z1 = jd_mul(z1, -7373), z2 = jd_mul(z2, -20995), z3 = jd_add(jd_mul(z3, -16069), z5), z4 = jd_add(jd_mul(z4, -3196), z5);
  tmp0 = jd_add(tmp0, jd_add(z1, z3)), tmp1 = jd_add(tmp1, jd_add(z2, z4));
  tmp2 = jd_add(tmp2, jd_add(z2, z3)), tmp3 = jd_add(tmp3, jd_add(z1, z4));
  o[0] = jd_descale(jd_add(tmp10, tmp3), descale), o[7 * ostride] = jd_descale(jd_sub(tmp10, tmp3), descale);
  o[ostride] = jd_descale(jd_add(tmp11, tmp2), descale), o[6 * ostride] = jd_descale(jd_sub(tmp11, tmp2), descale);
  o[2 * ostride] = jd_descale(jd_add(tmp12, tmp1), descale), o[5 * ostride] = jd_descale(jd_sub(tmp12, tmp1), descale);
  o[3 * ostride] = jd_descale(jd_add(tmp13, tmp0), descale), o[4 * ostride] = jd_descale(jd_sub(tmp13, tmp0), descale);
}

JD_HD uint8_t jd_range_limit(int32_t x) {
  const int32_t v = x & 1023;
  return (uint8_t)(v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896);
}

JD_HD void jd_idct_block(const int32_t *in, uint8_t *out, int pitch) {
  int32_t ws[64], row[8];
  for (int c = 0; c < 8; ++c) jd_idct_1d(in + c, 8, ws + c, 8, 13, 11);
  for (int r = 0; r < 8; ++r) {
    jd_idct_1d(ws + 8 * r, 1, row, 1, 13, 18);
    for (int c = 0; c < 8; ++c) out[(size_t)r * pitch + c] = jd_range_limit(row[c]);
  }
}

JD_HD uint8_t jd_clamp_u8(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// JFIF's YCbCr -> RGB in 16-bit fixed point (libjpeg's jdcolor): 1.402 = 91881 / 65536, 0.34414 = 22554, 0.71414 = 46802,
// 1.772 = 116130; the red and blue terms round to nearest on their own, the two green terms are added and rounded once.
JD_HD void jd_ycc_rgb(int y, int cb, int cr, uint8_t *rgb) {
  const int32_t b = cb - 128, r = cr - 128;
  rgb[0] = jd_clamp_u8(y + ((91881 * r + 32768) >> 16));
  rgb[1] = jd_clamp_u8(y + ((-22554 * b - 46802 * r + 32768) >> 16));
  rgb[2] = jd_clamp_u8(y + ((116130 * b + 32768) >> 16));
}

// The chrominance sample of pixel (x, y) from a plane of pitch `pitch` whose component is cw x ch: libjpeg's triangle filter
// (jdsample: h2v1 / h2v2 "fancy" upsampling), edges replicated at the component's own size; where cw <= 2 libjpeg repeats
// samples instead, and so does this.
JD_HD int jd_chroma_at(const uint8_t *pl, int pitch, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return pl[(size_t)y * pitch + x];
  const int i = x >> 1;
  if (vs == 1) {
    const uint8_t *row = pl + (size_t)y * pitch;
    const int v = row[i];
    if (cw <= 2) return v;
    if (x & 1) return i == cw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
    return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  const uint8_t *near = pl + (size_t)j * pitch;
  if (cw <= 2) return near[i];
  const int jf = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
  const uint8_t *far = pl + (size_t)jf * pitch;
  const int here = 3 * near[i] + far[i];
  if (x & 1) return i == cw - 1 ? (4 * here + 7) >> 4 : (3 * here + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
  return i == 0 ? (4 * here + 8) >> 4 : (3 * here + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}
