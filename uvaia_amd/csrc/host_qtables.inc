// host_qtables.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): everything the scans need from the
// query set -- query planes, recoded planes and ambiguity-word lists, column classes, rare columns, compressed and "dirty" query
// planes, the item stream of every super-tile of 64 queries -- built by host threads from the query rows and uploaded.
namespace {

int build_query_tables_host(uvaia_gpu_ctx *c, const uvaia_gpu_query *q, const uvaia_gpu_tuning &tn, const uint8_t *code_tab, int lo, int hi, const std::vector<uint8_t> &in_p)
{
#define OPENCHK(call) HIP_TRY(call, return fail(nullptr, code_, "%s failed: %s", #call, hipGetErrorString(e_)))      /* the caller closes the half-made context */
  const size_t row_words = (size_t)c->W4 * 4 * c->NQ;
  std::vector<uint32_t> qp((size_t)c->nq_pad * row_words, 0u);
  {
    std::atomic<int> first_bad(c->nq);
    std::vector<int> bad_byte((size_t)c->nq, 0);
    parallel_for(c->nq, [&](int i) {
      if (pack_query_row(code_tab, q->seq[i], c->nchar, lo, hi, nullptr, in_p.data(), c->acgt, c->NQ, qp.data() + (size_t)i * row_words, &bad_byte[(size_t)i])) {
        int cur = first_bad.load();
        while (i < cur && !first_bad.compare_exchange_weak(cur, i)) {}
      }
    });
    if (first_bad.load() < c->nq) {
      const int i = first_bad.load();
      return fail(nullptr, UVAIA_GPU_EALPHABET, "query %d holds byte 0x%02x outside the supported alphabet", i, bad_byte[(size_t)i]);
    }
  }
  if (int rc_ = c->tab.d_qp.reserve(nullptr, qp.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_qp, qp.data(), qp.size() * 4, hipMemcpyHostToDevice));
  c->tab.qtab[0] = {c->tab.d_qp, qp.size() * 4};
  {  // recoded planes and ambiguity-word lists for the two-counter path
    std::vector<int> ambq((size_t)c->nq * AMB_STRIDE, 0);
    if (!c->acgt) {
      const size_t row2 = (size_t)c->W4 * 16;
      std::vector<uint32_t> qp2((size_t)c->nq_pad * row2, 0u);
      parallel_for(c->nq, [&](int i) { for (int w = 0; w < c->W4 * 4; w++) {
        const uint32_t *s6 = qp.data() + (size_t)i * row_words + (size_t)w * 6;
        uint32_t *d4 = qp2.data() + (size_t)i * row2 + (size_t)w * 4;
        const uint32_t one = s6[5];
        d4[0] = (s6[1] | s6[3]) & one; d4[1] = (s6[2] | s6[3]) & one; d4[2] = one; d4[3] = s6[4];
        if (s6[4] & ~one) { int &cnt = ambq[(size_t)i * AMB_STRIDE]; if (cnt < AMB_CAP) ambq[(size_t)i * AMB_STRIDE + 1 + cnt] = w; cnt++; }
      } });
      if (int rc_ = c->tab.d_qp2.reserve(nullptr, qp2.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_qp2, qp2.data(), qp2.size() * 4, hipMemcpyHostToDevice));
      c->tab.qtab[1] = {c->tab.d_qp2, qp2.size() * 4};
    }
    {  // column classes and compressed/dirty query planes for scan3_kernel
      const int Wp = c->W4 * 4;
      auto QL = [&](int i, int w, int pl) -> uint32_t {          // (lo, hi, isACGT, valid-or-isACGT) of query i, word w
        if (c->acgt) { const uint32_t *s4 = qp.data() + (size_t)i * row_words + (size_t)w * 4; return pl == 3 ? s4[2] : s4[pl]; }
        const uint32_t *s6 = qp.data() + (size_t)i * row_words + (size_t)w * 6; const uint32_t one = s6[5];
        return pl == 0 ? ((s6[1] | s6[3]) & one) : pl == 1 ? ((s6[2] | s6[3]) & one) : pl == 2 ? one : s6[4];
      };
      std::vector<uint32_t> cls((size_t)Wp * 4, 0u);
      parallel_for(Wp, [&](int w) {
        uint32_t cL = 0, cH = 0, seen = 0, poly = 0;
        for (int i = 0; i < c->nq; i++) {
          const uint32_t qL = QL(i, w, 0), qH = QL(i, w, 1), qI = QL(i, w, 2);
          poly |= seen & qI & ((qL ^ cL) | (qH ^ cH));
          const uint32_t fresh = qI & ~seen;
          cL |= qL & fresh; cH |= qH & fresh; seen |= qI;
        }
        cls[(size_t)w * 4 + 0] = cL & ~poly; cls[(size_t)w * 4 + 1] = cH & ~poly; cls[(size_t)w * 4 + 2] = seen & ~poly; cls[(size_t)w * 4 + 3] = poly;
      });
      // Rare columns: polymorphic, but all except a few queries carry the same base (private mutations, sequencing noise: 95 % of
      // the polymorphic columns of the benchmark queries).  They are handled like constant columns with that base; the few
      // queries that differ are "dirty" there (their E bit is taken away by the usual items) and get the true comparison from a
      // sparse item on the gathered planes of the rare columns.  Dense work remains for the truly polymorphic columns only.
      std::vector<uint32_t> rmask((size_t)Wp, 0u);
      {
        c->tab.rare_max = tn.rare_max > 0 ? tn.rare_max : tn.rare_max < 0 ? 0 : (c->nq < 64 ? 0 : std::min(64, std::max(4, c->nq / 64)));
        if (c->fullscan || c->scan_variant != 2) c->tab.rare_max = 0;
      }
      if (c->tab.rare_max > 0) {
        parallel_for(Wp, [&](int w) {
          const uint32_t pm = cls[(size_t)w * 4 + 3];
          if (!pm) return;
          int cnt[32 * 4] = {0};
          for (int i = 0; i < c->nq; i++) {
            const uint32_t qL = QL(i, w, 0), qH = QL(i, w, 1);
            for (uint32_t m = QL(i, w, 2) & pm; m; m &= m - 1) { const int b = __builtin_ctz(m); cnt[(size_t)b * 4 + (((qL >> b) & 1u) | (((qH >> b) & 1u) << 1))]++; }
          }
          for (uint32_t m = pm; m; m &= m - 1) {
            const int b = __builtin_ctz(m);
            int major = 0, total = 0;
            for (int k = 0; k < 4; k++) { total += cnt[(size_t)b * 4 + k]; if (cnt[(size_t)b * 4 + k] > cnt[(size_t)b * 4 + major]) major = k; }
            if (total - cnt[(size_t)b * 4 + major] > c->tab.rare_max) continue;
            const uint32_t bit = 1u << b;
            cls[(size_t)w * 4 + 0] = (cls[(size_t)w * 4 + 0] & ~bit) | ((major & 1) ? bit : 0u);
            cls[(size_t)w * 4 + 1] = (cls[(size_t)w * 4 + 1] & ~bit) | ((major & 2) ? bit : 0u);
            cls[(size_t)w * 4 + 2] |= bit; cls[(size_t)w * 4 + 3] &= ~bit; rmask[(size_t)w] |= bit;
          }
        });
      }
      for (int w = 0; w < Wp; w++) { c->tab.NP += __builtin_popcount(cls[(size_t)w * 4 + 3]); c->tab.NR += __builtin_popcount(rmask[(size_t)w]); }
      c->tab.NP4 = ((c->tab.NP + 31) / 32 + 3) / 4;
      c->tab.NR4 = ((c->tab.NR + 31) / 32 + 3) / 4;
      // the compressed scan keeps a pair's deficit in 16 bits around SCAN3_BIAS: what the polymorphic and the rare columns can take away
      // has to stay below it (16 000 such columns of at most 49 000: no SARS-CoV-2 query set comes near); else the packed-plane scan
      if (c->scan_variant == 2 && (size_t)c->tab.NP4 * 128 + (size_t)c->tab.NR4 * 128 > SCAN3_BIAS - 256) c->scan_variant = 0;
      struct RareWord { int word; uint32_t m, l, h; };                  // one query's minority sites in one compressed word of the rare columns
      std::vector<std::vector<RareWord>> rare_q((size_t)c->nq_pad);
      std::vector<uint32_t> qrare((size_t)c->nq * std::max(c->tab.NR4, 1) * 12, 0u);
      const size_t prow = (size_t)std::max(c->tab.NP4, 1) * 16, crow = (size_t)c->W4 * 8;
      std::vector<uint32_t> qpl((size_t)c->nq_pad * prow, 0u), qcv((size_t)c->nq_pad * crow, 0u), flg((size_t)(c->nq_pad / 16) * c->W4 * 2, 0u);
      parallel_for(c->nq_pad / 16, [&](int tile_) { for (int i = tile_ * 16; i < tile_ * 16 + 16; i++) {   // a tile's 16 queries share flag words
        int k = 0, kr = 0;                                           // compressed bit position among the dense / the rare columns
        bool full = false;                                           // all 128 columns of the current word group are N/gap
        for (int w = 0; w < Wp; w++) {
          const bool real = i < c->nq;
          const uint32_t qL = real ? QL(i, w, 0) : 0u, qH = real ? QL(i, w, 1) : 0u, qI = real ? QL(i, w, 2) : 0u, qV = real ? QL(i, w, 3) : 0u;
          for (uint32_t m = cls[(size_t)w * 4 + 3]; m; m &= m - 1, k++) {
            const int b = __builtin_ctz(m);
            uint32_t *d = qpl.data() + (size_t)i * prow + (size_t)(k >> 7) * 16 + ((k >> 5) & 3);     // [p4][L,H,I,-][word of the group]
            d[0] |= ((qL >> b) & 1u) << (k & 31); d[4] |= ((qH >> b) & 1u) << (k & 31); d[8] |= ((qI >> b) & 1u) << (k & 31);
          }
          // dirty on a constant (or rare) column = not carrying the column's base there
          const uint32_t eqb = qI & ~((qL ^ cls[(size_t)w * 4 + 0]) | (qH ^ cls[(size_t)w * 4 + 1]));
          const uint32_t nI = ~eqb & cls[(size_t)w * 4 + 2], nV = ~qV;
          for (uint32_t m = rmask[(size_t)w]; m; m &= m - 1, kr++) {
            const int b = __builtin_ctz(m);
            if (real) { uint32_t *d = qrare.data() + ((size_t)i * c->tab.NR4 * 4 + (size_t)(kr >> 5)) * 3;
                        d[0] |= ((qL >> b) & 1u) << (kr & 31); d[1] |= ((qH >> b) & 1u) << (kr & 31); d[2] |= ((qI >> b) & 1u) << (kr & 31); }
            if (!real || !((qI >> b) & 1u) || ((eqb >> b) & 1u)) continue;          // only ACGT queries that differ from the majority
            if (rare_q[(size_t)i].empty() || rare_q[(size_t)i].back().word != (kr >> 5)) rare_q[(size_t)i].push_back({kr >> 5, 0u, 0u, 0u});
            RareWord &rw = rare_q[(size_t)i].back();
            rw.m |= 1u << (kr & 31); rw.l |= ((qL >> b) & 1u) << (kr & 31); rw.h |= ((qH >> b) & 1u) << (kr & 31);
          }
          qcv[(size_t)i * crow + (size_t)(w >> 2) * 8 + (w & 3)] = nI; qcv[(size_t)i * crow + (size_t)(w >> 2) * 8 + 4 + (w & 3)] = nV;
          uint32_t *fw = &flg[((size_t)(i / 16) * c->W4 + (w >> 2)) * 2];
          if (real && nI) fw[0] |= 1u << (i % 16);       // padding queries of the last tile are never read back: keep them "clean"
          if (real && nV) fw[0] |= 0x10000u << (i % 16);
          if ((w & 3) == 0) full = real;
          full = full && nI == cls[(size_t)w * 4 + 2] && nV == 0xFFFFFFFFu;
          if ((w & 3) == 3 && full) { fw[0] &= ~(0x10001u << (i % 16)); fw[1] |= 1u << (i % 16); }
        }
      } });
      for (int g = 0; g < c->W4; g++) {
        uint32_t u = 0;
        uint32_t uy = 0;
        for (int t = 0; t < c->nq_pad / 16; t++) { u |= flg[((size_t)t * c->W4 + g) * 2]; uy |= flg[((size_t)t * c->W4 + g) * 2 + 1]; }
        c->tab.need_e_groups += (u & 0xFFFFu) != 0; c->tab.need_v_groups += (u >> 16) != 0; c->tab.need_g_groups += uy != 0;
      }
      // Next to a running scan (8 blocks x 16.9 KB of LDS per CU) a replay block with the 22 KB query row fits once per CU, without
      // it seven times: with many queries the replay then waits for LDS, not for work (5.48 -> 5.04 ms per config[1] search).
      if (c->replay_lq < 0) c->replay_lq = (c->nq < 256) ? 1 : 0;
      if (int rc_ = c->tab.d_cls.reserve(nullptr, cls.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_cls, cls.data(), cls.size() * 4, hipMemcpyHostToDevice));
      if (int rc_ = c->tab.d_qrare.reserve(nullptr, qrare.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_qrare, qrare.data(), qrare.size() * 4, hipMemcpyHostToDevice));
      if (int rc_ = c->tab.d_rmask.reserve(nullptr, rmask.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_rmask, rmask.data(), rmask.size() * 4, hipMemcpyHostToDevice));
      c->tab.qtab[3] = {c->tab.d_cls, cls.size() * 4}; c->tab.qtab[4] = {c->tab.d_rmask, rmask.size() * 4}; c->tab.qtab[6] = {c->tab.d_qrare, qrare.size() * 4};
      {   // derive_all_kernel: word groups per wave and the bit positions its gathered columns start at
        int split[DERIVE_SPLIT_INTS];
        build_derive_split(cls.data(), rmask.data(), c->W4, split);
        if (int rc_ = c->tab.d_split.reserve(nullptr, DERIVE_SPLIT_INTS)) return rc_; OPENCHK(hipMemcpy(c->tab.d_split, split, sizeof split, hipMemcpyHostToDevice));
        c->tab.qtab[9] = {c->tab.d_split, sizeof split};
      }
      if (int rc_ = c->tab.d_qpl.reserve(nullptr, qpl.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_qpl, qpl.data(), qpl.size() * 4, hipMemcpyHostToDevice));
      c->tab.qtab[5] = {c->tab.d_qpl, qpl.size() * 4};
      // the item stream of every query tile (layout: see scan3_kernel)
      const int NWs = c->scan_NW, QS = 64;
      const uint32_t row_b = 256u * (uint32_t)c->scan_R;      // bytes of a query's counter row in a wave's LDS block: 64 lanes x R tiles x 4
      // one stream per super-tile of 64 queries (scan3_kernel: four waves share the counters and the stream)
      struct Rec { size_t at; uint32_t cost; };
      struct TileStream { std::vector<uint32_t> u; std::vector<Rec> rec, rare; };
      const int n_st = c->nq_pad / QS;
      std::vector<TileStream> ts((size_t)n_st);
      std::vector<uint8_t> rare_groups_needed((size_t)std::max(c->tab.NR4, 1), 0);
      parallel_for(n_st, [&](int st) {
        TileStream &S = ts[(size_t)st];
        std::vector<uint32_t> &strm = S.u;
        std::vector<int> full, gen, wrd[4];
        for (int g = 0; g < c->W4; g++) {
          full.clear(); gen.clear(); for (auto &w : wrd) w.clear();
          uint32_t wmask[64]; bool any_run = false;
          for (int ql = 0; ql < QS; ql++) {
            const int q = st * QS + ql, t = q / 16, b = q % 16;
            const uint32_t fx = flg[((size_t)t * c->W4 + g) * 2], fy = flg[((size_t)t * c->W4 + g) * 2 + 1];
            if ((fy >> b) & 1u) { full.push_back(ql); continue; }
            if (!(((fx | (fx >> 16)) >> b) & 1u)) continue;
            // a dirty query whose non-ACGT / invalid sites of this group all lie in ONE 32-column word (an isolated N or ambiguity
            // code: more than half of the partially dirty cases) gets a 4-dword "word item" instead of the 12-dword general one
            // ... and so does one whose other dirty words hold no valid query character at all (the edge of an N run: 88 % of what
            // would be general items for the benchmark queries): for such a "full" word the two counts are the reference's own
            // popcounts of E and V, which the scan has per record; the item carries the byte mask of those words (run item)
            const uint32_t *src = qcv.data() + (size_t)q * crow + (size_t)g * 8;
            int n_part = 0, part = 0, last_full = 0;
            uint32_t fm = 0u;
            for (int j = 0; j < 4; j++) {
              if (!(src[j] | src[4 + j])) continue;
              if (src[4 + j] == 0xFFFFFFFFu && src[j] == cls[(size_t)(g * 4 + j) * 4 + 2]) { last_full = j; fm |= 0xFFu << (8 * j); }
              else { n_part++; part = j; }
            }
            int jsel = -1;
            if (n_part == 1) jsel = part;
            else if (n_part == 0) { jsel = last_full; fm &= ~(0xFFu << (8 * last_full)); }     // (one to three full words: the last one is the item's own word)
            if (jsel >= 0) { wrd[jsel].push_back(ql); wmask[ql] = fm; any_run |= fm != 0u; } else gen.push_back(ql);
          }
          if (full.empty() && gen.empty() && wrd[0].empty() && wrd[1].empty() && wrd[2].empty() && wrd[3].empty()) continue;
          const size_t hdr = strm.size();
          const uint32_t n_full4 = (uint32_t)(full.size() + 3) / 4u;
          strm.push_back((uint32_t)g * 2048u | (any_run ? 1u : 0u));             // bit 0: some word item of the record is a run item
          strm.push_back(n_full4 | (uint32_t)gen.size() << 16);
          strm.push_back((uint32_t)wrd[0].size() | (uint32_t)wrd[1].size() << 8 | (uint32_t)wrd[2].size() << 16 | (uint32_t)wrd[3].size() << 24);
          strm.push_back(0u);
          for (int ql : full) strm.push_back((uint32_t)ql * row_b);
          while (strm.size() & 3) strm.push_back((uint32_t)QS * row_b);                         // scratch row
          for (int ql : gen) {
            const uint32_t *src = qcv.data() + (size_t)(st * QS + ql) * crow + (size_t)g * 8;
            strm.insert(strm.end(), src, src + 8);
            strm.push_back((uint32_t)ql * row_b); strm.push_back(0u); strm.push_back(0u); strm.push_back(0u);
          }
          for (int j = 0; j < 4; j++)
            for (int ql : wrd[j]) {
              const uint32_t *src = qcv.data() + (size_t)(st * QS + ql) * crow + (size_t)g * 8;
              strm.push_back(src[j]); strm.push_back(src[4 + j]); strm.push_back((uint32_t)ql * row_b); strm.push_back(wmask[ql]);
            }
          strm[hdr + 3] = (uint32_t)(strm.size() - hdr);
          S.rec.push_back({hdr, 60u + 4u * n_full4 + 30u * (uint32_t)gen.size() + 14u * (uint32_t)(wrd[0].size() + wrd[1].size() + wrd[2].size() + wrd[3].size())});
        }
        // the walk runs two headers ahead and takes a record's length from its header: a zero header of length 4 ends the group records
        strm.push_back(0u); strm.push_back(0u); strm.push_back(0u); strm.push_back(4u);
        strm.push_back(0u); strm.push_back(0u); strm.push_back(0u); strm.push_back(4u);
        // rare records: { byte offset of the rare group's planes in the tile's gathered planes, word-item counts (8 bits each), 0, 0 }
        // + items { sites, their lo bits, their hi bits, LDS offset } listed word by word
        for (int r4 = 0; r4 < c->tab.NR4; r4++) {
          uint32_t nw[4] = {0, 0, 0, 0};
          for (int ql = 0; ql < QS; ql++) for (const RareWord &rw : rare_q[(size_t)st * QS + ql]) if ((rw.word >> 2) == r4) nw[rw.word & 3]++;
          if (!(nw[0] | nw[1] | nw[2] | nw[3])) continue;
          S.rare.push_back({strm.size(), nw[0] + nw[1] + nw[2] + nw[3]});
          strm.push_back((uint32_t)(c->tab.NP4 + r4) * 3072u); strm.push_back(nw[0] | nw[1] << 8 | nw[2] << 16 | nw[3] << 24); strm.push_back(0u); strm.push_back(0u);
          for (int j = 0; j < 4; j++)
            for (int ql = 0; ql < QS; ql++) for (const RareWord &rw : rare_q[(size_t)st * QS + ql]) if (rw.word == r4 * 4 + j) {
              strm.push_back(rw.m); strm.push_back(rw.l); strm.push_back(rw.h); strm.push_back((uint32_t)ql * row_b);
            }
          rare_groups_needed[(size_t)r4] = 1;     // (a byte set to 1 by several threads)
        }
      });
      std::vector<uint32_t> strm, sdir((size_t)n_st * 4 * NWs, 0u);
      auto split4 = [NWs](const std::vector<Rec> &r, size_t base, size_t end_at, uint32_t *dir) {   // NW contiguous shares of about the same cost
        uint64_t total = 0;
        for (const Rec &x : r) total += x.cost;
        size_t i = 0; uint64_t done = 0;
        for (int w = 0; w < NWs; w++) {
          const size_t i0 = i;
          const uint64_t goal = total * (uint64_t)(w + 1) / (uint64_t)NWs;
          while (i < r.size() && (w == NWs - 1 || done + r[i].cost / 2 < goal)) { done += r[i].cost; i++; }
          dir[2 * w] = (uint32_t)(base + (i0 < r.size() ? r[i0].at : end_at));
          dir[2 * w + 1] = (uint32_t)(i - i0);
        }
      };
      for (int st = 0; st < n_st; st++) {
        const TileStream &S = ts[(size_t)st];
        const size_t base = strm.size(), zero_hdr = S.rec.empty() ? 0 : 0;
        (void)zero_hdr;
        // a wave without records still looks at two headers: point it at the zero headers that end the group records
        size_t end_at = S.u.size() - 8;
        for (const Rec &x : S.rare) { end_at = std::min(end_at, x.at - 8); break; }
        split4(S.rec, base, end_at, &sdir[(size_t)st * 4 * NWs]);
        split4(S.rare, base, S.u.size() - 8, &sdir[(size_t)st * 4 * NWs + 2 * NWs]);
        strm.insert(strm.end(), S.u.begin(), S.u.end());
      }
      for (uint8_t u : rare_groups_needed) c->tab.need_r_groups += u;
      strm.resize(strm.size() + 64, 0u);                                // the kernel prefetches items and headers past the end
      if (int rc_ = c->tab.d_stream.reserve(nullptr, strm.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_stream, strm.data(), strm.size() * 4, hipMemcpyHostToDevice));
      if (int rc_ = c->tab.d_sdir.reserve(nullptr, sdir.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_sdir, sdir.data(), sdir.size() * 4, hipMemcpyHostToDevice));
      c->tab.qtab[7] = {c->tab.d_stream, strm.size() * 4}; c->tab.qtab[8] = {c->tab.d_sdir, sdir.size() * 4};
    }
    if (int rc_ = c->tab.d_amb_q.reserve(nullptr, ambq.size())) return rc_; OPENCHK(hipMemcpy(c->tab.d_amb_q, ambq.data(), ambq.size() * sizeof(int), hipMemcpyHostToDevice));
    c->tab.qtab[2] = {c->tab.d_amb_q, ambq.size() * sizeof(int)};
  }
  return 0;
#undef OPENCHK
}

}  // namespace
