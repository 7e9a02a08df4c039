// The device JPEG decoder's whole scheme on the host, serially over lanes, from the functions the kernels are made of
// (csrc/jpeg_decode_core.h): for running under the host sanitizers on good and on damaged streams.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I video-diffusion-pipeline-parallel_amd/csrc tools/jpeg_decode_hostcheck.cpp -o jpeg_decode_hostcheck
//   jpeg_decode_hostcheck job.bin out.bin [job2.bin out2.bin ...]
//
// job.bin: 17 int32 header fields, int32 have_quant, int32 have_huff, 256 bytes of quantisation tables, 64 + 1024 bytes of DHT
// specifications (all as sp_jpeg_decode_plan takes them), then the entropy-coded segment.  out.bin: 8 int32 (error bits,
// fixed point reached, passes, clean bytes, markers, subsequences, longest interval, coefficients written), then, where the
// last is 1, the coefficients (int16) and the picture (h x w x 3 bytes).  Every buffer is allocated at exactly the size the
// library's layout gives it, so that a store or a load outside it is seen.  Exit status 0 whatever the stream holds; 2 for a
// job the plan refuses, 3 for a file that cannot be read or written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_decode_core.h"

static std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> data;
  FILE *f = fopen(path, "rb");
  if (!f) return data;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  return data;
}

static int run(const char *job_path, const char *out_path) {
  const std::vector<uint8_t> job = read_file(job_path);
  const size_t head = 19 * 4 + 256 + 64 + 1024;
  if (job.size() < head) return 3;
  int32_t fields[19];
  memcpy(fields, job.data(), sizeof fields);
  JdPlan *plan = new JdPlan();
  const char *why = "";
  if (fields[6] < 0 || (size_t)fields[6] != job.size() - head ||
      jd_make_plan(fields, job.data() + 76, fields[17], job.data() + 76 + 256, job.data() + 76 + 320, fields[18], plan, &why) != 0) {
    fprintf(stderr, "refused: %s\n", why);
    delete plan;
    return 2;
  }
  const JdParams &p = plan->p;
  const JdHuff *huff = plan->t.huff;
  JdLayout L;
  jd_layout(&p, &L);
  const uint8_t *seg = job.data() + head;
  int32_t meta[JD_M_WORDS] = {0};

  // 1. unstuff and split
  std::vector<uint32_t> words(L.clean_cap / 4);
  uint8_t *clean = (uint8_t *)words.data();
  std::vector<uint32_t> iv_start(p.n_iv + 1, 0), sub_first(p.n_iv + 1, 0);
  uint32_t at = 0, mk = 0;
  for (int i = 0; i < p.seg_len; ++i) {
    const int c = jd_classify(i ? seg[i - 1] : 0, seg[i], i + 1 < p.seg_len ? seg[i + 1] : -1);
    if (c & 4) meta[JD_M_ERROR] |= JD_E_MARKER;
    if (c & 1) {
      if (at < (uint32_t)p.seg_len) clean[at] = seg[i];
      ++at;
    } else if (c & 2) {
      if (seg[i + 1] != 0xD0 + (int)(mk & 7)) meta[JD_M_ERROR] |= JD_E_RST_ORDER;
      if (mk + 1 < (uint32_t)p.n_iv) iv_start[mk + 1] = at;
      ++mk;
    }
  }
  meta[JD_M_CLEAN] = (int32_t)at, meta[JD_M_MARKERS] = (int32_t)mk;
  iv_start[0] = 0, iv_start[p.n_iv] = at;
  if (mk != (uint32_t)(p.n_iv - 1)) meta[JD_M_ERROR] |= JD_E_RST_COUNT;

  std::vector<int16_t> coef((size_t)p.total_mcus * p.bpm * 64, 0);
  std::vector<uint8_t> rgb((size_t)p.w * p.h * 3, 0);
  if (!meta[JD_M_ERROR]) {
    uint32_t subs = 0, longest = 0;
    for (int k = 0; k < p.n_iv; ++k) {
      const uint32_t lo = iv_start[k] < at ? iv_start[k] : at, hi = iv_start[k + 1] < at ? iv_start[k + 1] : at;
      const uint32_t bits = hi > lo ? 8u * (hi - lo) : 0u, ns = (bits + (uint32_t)p.subseq_bits - 1) / (uint32_t)p.subseq_bits;
      sub_first[k] = subs, subs += ns;
      if (ns > longest) longest = ns;
    }
    sub_first[p.n_iv] = subs;
    meta[JD_M_SUBS] = (int32_t)subs, meta[JD_M_LONGEST] = (int32_t)longest;
    if (subs > (uint32_t)p.max_sub) {                            // (the layout's bound; cannot happen)
      delete plan;
      return 3;
    }

    // 2. passes until one changes nothing
    std::vector<JdRec> rec[2] = {std::vector<JdRec>(p.max_sub), std::vector<JdRec>(p.max_sub)};
    std::vector<int> interval(subs);
    for (int k = 0; k < p.n_iv; ++k)
      for (uint32_t g = sub_first[k]; g < sub_first[k + 1]; ++g) interval[g] = k;
    for (int pass = 0; pass <= (int)longest + 1; ++pass) {
      int changed = 0;
      for (uint32_t g = 0; g < subs; ++g) {
        const int k = interval[g];
        const uint32_t j = g - sub_first[k];
        const JdRec none = {0, 0, 0, 0, 0, 0};
        changed += jd_lane_pass(words.data(), 8u * iv_start[k], 8u * iv_start[k + 1], j, pass, huff, &p,
                                pass > 0 && j > 0 ? &rec[(pass + 1) & 1][g - 1] : &none, pass > 0 ? &rec[(pass + 1) & 1][g] : &none,
                                &rec[pass & 1][g]);
      }
      meta[JD_M_PASSES] = pass + 1;
      if (!changed) {
        meta[JD_M_FIXED] = 1;
        break;
      }
    }

    // 3. coefficients
    if (meta[JD_M_FIXED]) {
      const std::vector<JdRec> &r = rec[(meta[JD_M_PASSES] - 1) & 1];      // the last pass: its starts are the true exits
      std::vector<uint32_t> lane_first(p.max_sub + 1, 0);
      uint32_t total = 0;
      for (uint32_t g = 0; g < subs; ++g) {
        lane_first[g] = total, total += r[g].nblk;
        if (r[g].err) meta[JD_M_ERROR] |= JD_E_CODE;
      }
      lane_first[subs] = total;
      for (int k = 0; k < p.n_iv; ++k)
        if (lane_first[sub_first[k + 1]] - lane_first[sub_first[k]] != (uint32_t)jd_interval_mcus(&p, k) * (uint32_t)p.bpm)
          meta[JD_M_ERROR] |= JD_E_BLOCKS;
      if (!meta[JD_M_ERROR]) {
        for (uint32_t g = 0; g < subs; ++g) {
          const int k = interval[g];
          const uint32_t j = g - sub_first[k], bit0 = 8u * iv_start[k], end_bits = 8u * iv_start[k + 1];
          const uint64_t nominal = (uint64_t)bit0 + ((uint64_t)j + 1) * (uint32_t)p.subseq_bits;
          const uint32_t base = (uint32_t)k * (uint32_t)p.restart * (uint32_t)p.bpm;
          JdLane ln;
          ln.pos = r[g].in_pos, ln.blk = (int32_t)(r[g].in_st >> 8), ln.zz = (int32_t)(r[g].in_st & 255), ln.nblk = 0;
          jd_lane_run(words.data(), end_bits, nominal < end_bits ? (uint32_t)nominal : end_bits, huff, &p, &ln, coef.data(),
                      base + lane_first[g] - lane_first[sub_first[k]], base + (uint32_t)jd_interval_mcus(&p, k) * (uint32_t)p.bpm);
        }
        int32_t pred[3] = {0, 0, 0};
        for (int m = 0; m < p.total_mcus; ++m) {
          if (m % p.restart == 0) pred[0] = pred[1] = pred[2] = 0;
          for (int b = 0; b < p.bpm; ++b) {
            int16_t &dc = coef[((size_t)m * p.bpm + b) * 64];
            int32_t &pr = pred[p.blk_comp[b]];
            pr = jd_add(pr, dc);
            dc = (int16_t)(pr < -32768 ? -32768 : pr > 32767 ? 32767 : pr);
          }
        }
        meta[JD_M_COEF_DONE] = 1;
      }
    }

    // 4. pixels
    if (meta[JD_M_COEF_DONE]) {
      static const uint8_t zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
      const size_t luma = (size_t)L.luma_w * L.luma_h, chroma = (size_t)L.chroma_w * L.chroma_h;
      std::vector<uint8_t> planes(luma + 2 * chroma);
      for (int m = 0; m < p.total_mcus; ++m)
        for (int b = 0; b < p.bpm; ++b) {
          const int c = p.blk_comp[b], mr = m / p.mcu_cols, mc = m % p.mcu_cols;
          const int pitch = c ? L.chroma_w : L.luma_w;
          uint8_t *dst = c ? planes.data() + luma + (size_t)(c - 1) * chroma + (size_t)mr * 8 * pitch + (size_t)mc * 8
                           : planes.data() + (size_t)(mr * p.vs + b / p.hs) * 8 * pitch + (size_t)(mc * p.hs + b % p.hs) * 8;
          int32_t in[64];
          for (int k = 0; k < 64; ++k)
            in[zigzag[k]] = (int32_t)coef[((size_t)m * p.bpm + b) * 64 + k] * (int32_t)plan->t.quant[p.comp_tq[c]][zigzag[k]];
          jd_idct_block(in, dst, pitch);
        }
      const int cw = (p.w + p.hs - 1) / p.hs, ch = (p.h + p.vs - 1) / p.vs;
      for (int y = 0; y < p.h; ++y)
        for (int x = 0; x < p.w; ++x) {
          uint8_t *out = rgb.data() + ((size_t)y * p.w + x) * 3;
          const int lum = planes[(size_t)y * L.luma_w + x];
          if (p.ncomp == 1) out[0] = out[1] = out[2] = (uint8_t)lum;
          else
            jd_ycc_rgb(lum, jd_chroma_at(planes.data() + luma, L.chroma_w, cw, ch, p.hs, p.vs, x, y),
                       jd_chroma_at(planes.data() + luma + chroma, L.chroma_w, cw, ch, p.hs, p.vs, x, y), out);
        }
    }
  }

  FILE *f = fopen(out_path, "wb");
  if (!f) return 3;
  const int32_t status[8] = {meta[JD_M_ERROR],   meta[JD_M_FIXED], meta[JD_M_PASSES],  meta[JD_M_CLEAN],
                             meta[JD_M_MARKERS], meta[JD_M_SUBS],  meta[JD_M_LONGEST], meta[JD_M_COEF_DONE]};
  fwrite(status, sizeof status, 1, f);
  if (meta[JD_M_COEF_DONE]) {
    fwrite(coef.data(), sizeof(int16_t), coef.size(), f);
    fwrite(rgb.data(), 1, rgb.size(), f);
  }
  fclose(f);
  delete plan;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc % 2 != 1) {
    fprintf(stderr, "usage: %s job.bin out.bin [job2.bin out2.bin ...]\n", argv[0]);
    return 3;
  }
  int worst = 0;
  for (int i = 1; i + 1 < argc; i += 2) {
    const int rc = run(argv[i], argv[i + 1]);
    if (rc > worst) worst = rc;
  }
  return worst;
}
