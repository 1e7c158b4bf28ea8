// wfa_align_body.inc -- the body of the aligner's kernel, included by uvaia_align.hip once per kernel: wfa_align_kernel (INS = false) and
// wfa_align_insertions_kernel (INS = true, `ins` says where the insertion records go).  The including kernel declares `constexpr bool INS`,
// `const InsOut ins` and the parameters named below.  It is text inside the kernel and not a function the kernels call: the parameter struct
// P then stays a kernel argument that is read where it is used, and wfa_align_kernel compiles to the code it had before the records
// existed, instruction for instruction (a templated __device__ function, always inlined, was built first: P arrived in registers loaded at
// the kernel's entry, and the same source gave 71 instructions fewer and 157 instead of 152 spilled SGPRs).
//
// parameters: ref, plen, seqs, seq_off, todo, n_todo, aln, aln_pitch, score_out, status_out, cells_out, pool, ctl, stack, next_query, P
  __shared__ int ring[RING][HDR_INTS];
  __shared__ int own[MAX_OWN];
  __shared__ uint32_t hdr_page[MAX_HDR_PAGES];
  __shared__ int wsync[2][NW][2];
  __shared__ int dend[2][2][64];           // distance to the end cell of a wavefront's first and last 64 diagonals (for the reduction)
  __shared__ int bc[2];
  // The wavefronts a step reads -- M of score - x and score - o - e, I and D of score - e -- are those of the last few steps: they stay
  // in LDS (offset + 16 in 16 bits: the null offset is 6) as long as they are at most WL wide, and the history in memory is written
  // without being waited for.  A step then costs LDS latency plus one round trip for the characters of the extension.
  __shared__ uint16_t lm[RM][WL], li[RID][WL], ld[RID][WL];
  const int tid = threadIdx.x, lane = tid & 63, wave = rfl(tid >> 6);
  const int chunk_log2 = ctl->chunk_log2;
  const unsigned chunk_words = 1u << chunk_log2;
  const size_t home_base = (size_t)(2 * blockIdx.x) << chunk_log2, ring_base = (size_t)(2 * blockIdx.x + 1) << chunk_log2;
  // the I and D wavefronts a step reads are those of score - e, at most e / gcd steps back: more of them than LDS slots, and every step
  // keeps a copy of its I and D in memory
  const bool id_deep = P.e / P.g >= RID;
  unsigned long long cells_total = 0;

  for (;;) {
    if (tid == 0) bc[0] = atomicAdd(next_query, 1);
    __syncthreads();
    const int qi = rfl(bc[0]);                                // (read back from LDS: the same in every lane, and the compiler should know)
    if (qi >= n_todo) break;                                  // every wave of every block reaches this: the counter only grows
    const int q = todo ? todo[qi] : qi;
    const uint8_t *text = seqs + seq_off[q];
    const int tlen = (int)(seq_off[q + 1] - seq_off[q]);
    const int alignment_k = tlen - plen;
    uint8_t *row = aln + (size_t)q * aln_pitch;

    for (int i = tid; i < RING * HDR_INTS; i += TPB) (&ring[0][0])[i] = 0;
    __syncthreads();

    // bump allocation inside the current chunk; every thread keeps the same state
    size_t cur_base = home_base;
    unsigned cur_used = 0, ring_pos = 0, widest16 = 16;
    int n_own = 0;
    unsigned long long cells = 0;
    int score = 0, status = ST_OK, step = 0, cslot = 0, cislot = 0;      // cslot = step mod RM, cislot = step mod RID
    bool reached = false;

    auto take = [&](unsigned words, size_t &at) -> bool {    // `words` (a multiple of 16, at most a chunk) of the query's memory; false = the pool is empty
      if (cur_used + words > chunk_words) {
        __syncthreads();
        if (tid == 0) {
          int id = -1;
          if (n_own < MAX_OWN) {
            pool_lock(ctl);
            const int top = atomicAdd(&ctl->top, 0);
            if (top > 0) { id = atomicAdd(&stack[top - 1], 0); atomicExch(&ctl->top, top - 1); }
            pool_unlock(ctl);
            if (id >= 0) own[n_own] = id;
          }
          bc[1] = id;
        }
        __syncthreads();
        const int id = rfl(bc[1]);
        if (id < 0) return false;
        n_own++;
        cur_base = (size_t)id << chunk_log2; cur_used = 0;
      }
      at = cur_base + cur_used;
      cur_used += words;
      return true;
    };

    // ---------------- forward: one step per score ----------------
    for (;;) {
      if (score / HDR_PAGE_SCORES != (score - P.g) / HDR_PAGE_SCORES || score == 0) {     // a new page of headers
        const int page = score / HDR_PAGE_SCORES;
        size_t at = 0;
        if (page >= MAX_HDR_PAGES) { status = ST_HDRPAGES; break; }
        if (!take(HDR_PAGE_SCORES * HDR_INTS, at)) { status = ST_OVERFLOW; break; }
        if (tid == 0) hdr_page[page] = (uint32_t)(at >> 4);
        __syncthreads();
      }
      // the headers of the three source scores: the same for every lane, kept in scalar registers (a score below zero has none; where
      // the arrays lie in memory -- off16, w, id16 -- is looked up only by a step that has to read a source from there)
      auto load = [&](int s) -> Hdr {
        Hdr h{};
        if (s >= 0) { const int *r = ring[s & (RING - 1)]; h.lo = rfl(r[0]); h.hi = rfl(r[1]); h.lo_base = rfl(r[2]); h.flags = rfl(r[3]); h.res = rfl(r[7]); }
        return h;
      };
      const Hdr hs = load(score - P.x), hg = load(score - P.oe), he = load(score - P.e);
      const bool n_sub = !(hs.flags & 1), n_gap = !(hg.flags & 1), n_i = !(he.flags & 2), n_d = !(he.flags & 4);
      const bool have = score == 0 || !(n_sub && n_gap && n_i && n_d);
      int lo = 0, hi = 0;
      if (score > 0 && have) {
        lo = min(min(n_sub ? 1 : hs.lo, n_gap ? 1 : hg.lo), min(n_i ? 1 : he.lo, n_d ? 1 : he.lo)) - 1;
        hi = max(max(n_sub ? -1 : hs.hi, n_gap ? -1 : hg.hi), max(n_i ? -1 : he.hi, n_d ? -1 : he.hi)) + 1;
      }
      int *hdr_out = reinterpret_cast<int *>(pool + ((size_t)hdr_page[score / HDR_PAGE_SCORES] << 4)) + (size_t)(score & (HDR_PAGE_SCORES - 1)) * HDR_INTS;
      int *ring_out = ring[score & (RING - 1)];
      if (!have) {
        // every wave writes the (identical) ring entry it is going to read: no barrier for it; the header in memory is for the backtrace
        if (lane < HDR_INTS) { ring_out[lane] = 0; if (wave == 0) hdr_out[lane] = 0; }
      } else {
        const bool has_i = score > 0 && ((hg.flags & 1) || (he.flags & 2)), has_d = score > 0 && ((hg.flags & 1) || (he.flags & 4));
        const int w = hi - lo + 1, w16 = w16_of(w);
        const unsigned hist_words = (unsigned)w16 + (unsigned)w16_of((w + 3) / 4);
        // where the wavefronts of this step and of its sources live
        const bool fits = w <= WL && tlen + step + 32 < 65535;              // offsets grow by at most one per step beyond tlen
        // LDS slots: this step's (cslot, cislot: step mod RM, step mod RID, kept as running counters) and, d steps back, its sources'
        const int d_s = step - (hs.res - 1), d_g = step - (hg.res - 1), d_e = step - (he.res - 1);
        const bool lds_s = hs.res && d_s < RM, lds_g = hg.res && d_g < RM, lds_e = he.res && d_e < RID;
        const int slot_s = lds_s ? (cslot >= d_s ? cslot - d_s : cslot - d_s + RM) : 0, slot_g = lds_g ? (cslot >= d_g ? cslot - d_g : cslot - d_g + RM) : 0;
        const int slot_e = lds_e ? (cislot >= d_e ? cislot - d_e : cislot - d_e + RID) : 0;
        const bool sources_in_lds = (!(hs.flags & 1) || lds_s) && (!(hg.flags & 1) || lds_g) && (!(he.flags & 6) || lds_e);
        // The step proper, compiled twice.  LDS_ONLY: the usual step -- this wavefront fits in LDS, so do all it reads, all five source
        // wavefronts exist, and I and D need no copy in memory: nothing but the history of the backtrace leaves the CU, and none of the
        // bookkeeping of the other kind of step (positions in the ring chunk, pointers to sources in memory, which of them to wait for,
        // which wavefronts there are at all) is executed.  Returns true when the forward pass has to stop (status set).
        const bool all_sources = score > 0 && (hs.flags & 1) && (hg.flags & 1) && (he.flags & 6) == 6;
        auto step_body = [&](auto lds_only_tag) -> bool {
          constexpr bool LDS_ONLY = decltype(lds_only_tag)::value;
          const bool resident = LDS_ONLY || fits, some = LDS_ONLY || score > 0, with_i = LDS_ONLY || has_i, with_d = LDS_ONLY || has_d;
          auto inside = [&](const Hdr &h, int bit, int k) -> bool { return LDS_ONLY ? (k >= h.lo && k <= h.hi) : in_range(h, bit, k); };
          size_t id_at = 0;
          if (!LDS_ONLY) {
            // the ring chunk keeps the I and D wavefronts of the last e + 1 steps: e + 2 pairs of the widest one must fit (one is lost to the wrap)
            widest16 = max(widest16, (unsigned)w16);
            if ((unsigned long long)(P.e + 2) * 2ull * widest16 > chunk_words || hist_words > chunk_words) { status = ST_TOOWIDE; return true; }
            if (ring_pos + 2u * (unsigned)w16 > chunk_words) ring_pos = 0;
            id_at = ring_base + ring_pos;
            ring_pos += 2u * (unsigned)w16;
          }
          size_t m_at = 0;
          if (!take(hist_words, m_at)) { status = ST_OVERFLOW; return true; }
          cells += (unsigned)w;
          const bool id_to_memory = !LDS_ONLY && (!resident || id_deep);      // (more existing scores between s - e and s than LDS slots: keep a copy)
          const bool all_lds = LDS_ONLY || sources_in_lds;
          // a source that left LDS is read from memory, where its step wrote it without waiting: make those stores complete first
          if (!LDS_ONLY && (((hs.flags & 1) && hs.res && !lds_s) || ((hg.flags & 1) && hg.res && !lds_g) || ((he.flags & 6) && he.res && !lds_e))) __syncthreads();
          uint32_t *out_m = pool + m_at, *out_i = pool + id_at, *out_d = out_i + w16;
          uint8_t *out_c = reinterpret_cast<uint8_t *>(out_m + w16);
          // sources in memory (a step that is not all_lds): M of score - x, M of score - o - e, I and D of score - e
          auto mem_m = [&](int s_, const Hdr &h_) -> const uint32_t * { return pool + ((size_t)(uint32_t)ring[s_ & (RING - 1)][4] << 4) - h_.lo_base; };
          auto mem_i = [&](int s_, const Hdr &h_) -> const uint32_t * { return pool + ((size_t)(uint32_t)ring[s_ & (RING - 1)][6] << 4) - h_.lo_base; };
          int min_distance = max(plen, tlen);
          bool hit_end = false;
          // A cell in two halves.  front: its offset before the extension (five offsets from LDS, I and D stored) and the request for the
          // first eight characters of either sequence; back: the extension and the stores.  A wave takes its diagonals WFA_GROUP x 64 at
          // a time, all fronts before the first back: one LDS and one memory round trip per group instead of one per 64 diagonals.
          struct Cell { int k, m; unsigned code; bool act, go; unsigned long long x, y; };
          auto front = [&](int k0) -> Cell {
            Cell c;
            const int k = k0 + lane;
            const bool act = k <= hi;
            int m = 0;
            unsigned code = C_MISMATCH;
            if (some) {
              const bool in_s = inside(hs, 0, k), in_gm = inside(hg, 0, k - 1), in_gp = inside(hg, 0, k + 1), in_i = inside(he, 1, k - 1), in_d = inside(he, 2, k + 1);
              int r_s, r_gm, r_gp, r_i, r_d;
              if (all_lds) {     // the usual case: five unconditional LDS reads at clamped positions, the range tests as selects (no branches)
                const int xs = min(max(k - hs.lo_base, 0), WL - 1), xm = min(max(k - 1 - hg.lo_base, 0), WL - 1), xp = min(max(k + 1 - hg.lo_base, 0), WL - 1);
                const int xi = min(max(k - 1 - he.lo_base, 0), WL - 1), xd = min(max(k + 1 - he.lo_base, 0), WL - 1);
                const int a_s = (int)lm[slot_s][xs] - 16, a_m = (int)lm[slot_g][xm] - 16, a_p = (int)lm[slot_g][xp] - 16, a_i = (int)li[slot_e][xi] - 16, a_d = (int)ld[slot_e][xd] - 16;
                r_s = in_s ? a_s : WFA_NULL; r_gm = in_gm ? a_m : WFA_NULL; r_gp = in_gp ? a_p : WFA_NULL; r_i = in_i ? a_i : WFA_NULL; r_d = in_d ? a_d : WFA_NULL;
              } else {
                const uint32_t *ms = (hs.flags & 1) && !lds_s ? mem_m(score - P.x, hs) : pool, *mg = (hg.flags & 1) && !lds_g ? mem_m(score - P.oe, hg) : pool;
                const uint32_t *ie = (he.flags & 6) && !lds_e ? mem_i(score - P.e, he) : pool, *de = ie + ((he.flags & 6) && !lds_e ? w16_of(ring[(score - P.e) & (RING - 1)][5]) : 0);
                r_s  = in_s  ? (lds_s ? (int)lm[slot_s][k - hs.lo_base] - 16     : (int)ms[k])     : WFA_NULL;
                r_gm = in_gm ? (lds_g ? (int)lm[slot_g][k - 1 - hg.lo_base] - 16 : (int)mg[k - 1]) : WFA_NULL;
                r_gp = in_gp ? (lds_g ? (int)lm[slot_g][k + 1 - hg.lo_base] - 16 : (int)mg[k + 1]) : WFA_NULL;
                r_i  = in_i  ? (lds_e ? (int)li[slot_e][k - 1 - he.lo_base] - 16 : (int)ie[k - 1]) : WFA_NULL;
                r_d  = in_d  ? (lds_e ? (int)ld[slot_e][k + 1 - he.lo_base] - 16 : (int)de[k + 1]) : WFA_NULL;
              }
              // the five predecessors as the backtrace sees them (a "+ 1" belongs to a fetched value only)
              const int v_sub = in_s ? r_s + 1 : WFA_NULL, v_io = in_gm ? r_gm + 1 : WFA_NULL, v_ie = in_i ? r_i + 1 : WFA_NULL, v_do = r_gp, v_de = r_d;
              m = v_sub;
              if (with_i) { const int ins = max(r_gm, r_i) + 1; if (act) { if (resident) li[cislot][k - lo] = (uint16_t)(ins + 16); if (id_to_memory) out_i[k - lo] = (uint32_t)ins; } m = max(m, ins); }
              if (with_d) { const int del = max(r_gp, r_d);     if (act) { if (resident) ld[cislot][k - lo] = (uint16_t)(del + 16); if (id_to_memory) out_d[k - lo] = (uint32_t)del; } m = max(m, del); }
              const int bt = max(v_sub, max(max(v_io, v_ie), max(v_do, v_de)));
              code = bt == v_de ? C_DEL_EXT : bt == v_do ? C_DEL_OPEN : bt == v_ie ? C_INS_EXT : bt == v_io ? C_INS_OPEN : C_MISMATCH;   // the backtrace's tie order
              code |= (v_ie >= v_io ? C_I_EXT : 0) | (v_de >= v_do ? C_D_EXT : 0);
            }
            // exact extension along the diagonal (paper algorithm 2): eight characters per lane in one round trip (the loads may run up to
            // seven bytes past a sequence: both buffers are padded) ...
            const int v = m - k, h = m;
            c.k = k; c.m = m; c.code = code; c.act = act;
            c.go = act && (unsigned)h < (unsigned)tlen && (unsigned)v < (unsigned)plen;
            c.x = 0ull; c.y = 0ull;
            if (c.go) { __builtin_memcpy(&c.x, ref + v, 8); __builtin_memcpy(&c.y, text + h, 8); }
            return c;
          };
          auto back = [&](const Cell &c, int k0) {
            const int k = c.k;
            int m = c.m, v = m - k, h = m;
            bool go = c.go;
            {   // (no branch around this: a wait for the characters that a path can skip makes the next cells wait for this cell's stores)
              const unsigned long long d = c.x ^ c.y;
              const int nmat = go ? min(d ? (int)(__builtin_ctzll(d) >> 3) : 8, min(plen - v, tlen - h)) : 0;
              v += nmat; h += nmat; m += nmat;
              go = go && nmat == 8 && v < plen && h < tlen;
            }
            // ... longer runs by the whole wave, 1 024 characters per round trip
            unsigned long long more = __ballot(go);
            while (more) {
              const int j = __builtin_ctzll(more);
              more &= more - 1;
              const int vj = __shfl(v, j), hj = __shfl(h, j);
              int ext = 0;
              for (;;) {
                unsigned long long part[2];
                int nm_[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                  const int pv = vj + ext + (u * 64 + lane) * 8, ph = hj + ext + (u * 64 + lane) * 8;
                  nm_[u] = (pv < plen && ph < tlen) ? min(matching_prefix8(ref + pv, text + ph), min(plen - pv, tlen - ph)) : 0;
                  part[u] = __ballot(nm_[u] < 8);
                }
                if (part[0]) { const int l = __builtin_ctzll(part[0]); ext += 8 * l + __shfl(nm_[0], l); break; }
                if (part[1]) { const int l = __builtin_ctzll(part[1]); ext += 512 + 8 * l + __shfl(nm_[1], l); break; }
                ext += 1024;
              }
              if (lane == j) m += ext;
            }
            const int dk_ = c.act ? dist_to_end(plen, tlen, m, k) : 0x7fffffff;
            if (k0 == lo) dend[step & 1][0][lane] = dk_;
            if (k0 + 64 > hi) dend[step & 1][1][lane] = dk_;
            if (c.act) {
              if (resident) lm[cslot][k - lo] = (uint16_t)(m + 16);
              out_m[k - lo] = (uint32_t)m;
              out_c[k - lo] = (uint8_t)c.code;
              min_distance = min(min_distance, dk_);
              if (k == alignment_k && m >= tlen) hit_end = true;
            }
          };
          for (int k0 = lo + 64 * wave; k0 <= hi; k0 += WFA_GROUP * TPB) {
            Cell c[WFA_GROUP];
#pragma unroll
            for (int g = 0; g < WFA_GROUP; g++) if (k0 + g * TPB <= hi) c[g] = front(k0 + g * TPB);
            __builtin_amdgcn_sched_barrier(0);                   // (the scheduler would pair every front with its back again)
#pragma unroll
            for (int g = 0; g < WFA_GROUP; g++) if (k0 + g * TPB <= hi) back(c[g], k0 + g * TPB);
          }
          min_distance = wave_min_dpp(min_distance);
          const bool wave_hit = __any(hit_end);
          if (lane == 0) { wsync[step & 1][wave][0] = min_distance; wsync[step & 1][wave][1] = wave_hit ? 1 : 0; }
          if (resident) lds_barrier(); else __syncthreads();      // the one barrier of a step: offsets stored by other waves are read from here on
          min_distance = wsync[step & 1][0][0]; reached = wsync[step & 1][0][1] != 0;
#pragma unroll
          for (int u = 1; u < NW; u++) { min_distance = min(min_distance, wsync[step & 1][u][0]); reached = reached || wsync[step & 1][u][1] != 0; }
          min_distance = rfl(min_distance); reached = rfl(reached ? 1 : 0) != 0;     // uniform: the loop over the scores is a scalar loop
          const int par = step & 1;
          step++;
          // adaptive reduction (paper section 2.4): trim both ends of a long wavefront, never across the end cell's diagonal.
          // Every wave computes the same limits for itself, as a rule from the two ends' distances in LDS.
          int rlo = lo, rhi = hi;
          if (P.min_wf_len > 0 && w >= P.min_wf_len) {
            const int top_limit = min(alignment_k - 1, hi);
            if (lo < top_limit) {
              rlo = top_limit;
              const unsigned long long b0 = __ballot(lo + lane < top_limit && dend[par][0][lane] - min_distance <= P.max_dist_thr);
              if (b0) rlo = lo + __builtin_ctzll(b0);
              else for (int k0 = lo + 64; k0 < top_limit; k0 += 64) {
                const int k = k0 + lane;
                const bool keep = k < top_limit && dist_to_end(plen, tlen, resident ? (int)lm[cslot][k - lo] - 16 : (int)out_m[k - lo], k) - min_distance <= P.max_dist_thr;
                const unsigned long long b = __ballot(keep);
                if (b) { rlo = k0 + __builtin_ctzll(b); break; }
              }
            }
            const int bottom_limit = max(alignment_k + 1, rlo);
            if (hi > bottom_limit) {
              rhi = bottom_limit;
              const int kh = lo + ((hi - lo) / 64) * 64;                  // first diagonal of the chunk that holds hi
              const unsigned long long b0 = __ballot(kh + lane <= hi && kh + lane > bottom_limit && dend[par][1][lane] - min_distance <= P.max_dist_thr);
              if (b0) rhi = kh + 63 - __builtin_clzll(b0);
              else for (int k0 = kh - 1; k0 > bottom_limit; k0 -= 64) {
                const int k = k0 - lane;
                const bool keep = k > bottom_limit && dist_to_end(plen, tlen, resident ? (int)lm[cslot][k - lo] - 16 : (int)out_m[k - lo], k) - min_distance <= P.max_dist_thr;
                const unsigned long long b = __ballot(keep);
                if (b) { rhi = k0 - __builtin_ctzll(b); break; }
              }
            }
          }
          if (lane < HDR_INTS) {
            const int flags = 1 | (has_i ? 2 : 0) | (has_d ? 4 : 0);
            const int val = lane == 0 ? rlo : lane == 1 ? rhi : lane == 2 ? lo : lane == 3 ? flags : lane == 4 ? (int)(uint32_t)(m_at >> 4) : lane == 5 ? w : lane == 6 ? (int)(uint32_t)(id_at >> 4) : (resident ? step : 0);
            ring_out[lane] = val;
            if (wave == 0) hdr_out[lane] = val;
          }
          cslot = cslot + 1 == RM ? 0 : cslot + 1; cislot = cislot + 1 == RID ? 0 : cislot + 1;
          return false;
        };
        if ((fits && all_sources && sources_in_lds && !id_deep) ? step_body(BoolTag<true>()) : step_body(BoolTag<false>())) break;
      }
      if (reached) break;
      score += P.g;                                             // scores that are no multiple of gcd(x, o + e, e) have no wavefront (and no header: never looked up)
      if (score > P.max_score) { status = ST_MAXSCORE; break; }
    }
    __syncthreads();                                            // headers in memory, last offsets: visible to the backtrace
    // ---------------- backtrace + projection on the reference's columns (src/align.c:366-390): wave 0 ----------------
    if (status == ST_OK && wave == 0) {
      auto hdr_of = [&](int s, Hdr &h) {
        const int *r = reinterpret_cast<const int *>(pool + ((size_t)hdr_page[s / HDR_PAGE_SCORES] << 4)) + (size_t)(s & (HDR_PAGE_SCORES - 1)) * HDR_INTS;
        h.lo = r[0]; h.hi = r[1]; h.lo_base = r[2]; h.flags = r[3]; h.off16 = (uint32_t)r[4]; h.w = r[5];
      };
      auto m_of = [&](const Hdr &h, int k) { return (int)pool[((size_t)h.off16 << 4) + (size_t)(k - h.lo_base)]; };
      auto code_of = [&](const Hdr &h, int k) { return (int)reinterpret_cast<const uint8_t *>(pool + ((size_t)h.off16 << 4) + w16_of(h.w))[k - h.lo_base]; };
      auto cell_ok = [&](const Hdr &h, int k) { return (h.flags & 1) && k >= h.lo_base && k < h.lo_base + h.w; };
      int s = score, k = alignment_k, state = 0;              // state: 0 = M, 1 = I, 2 = D
      Hdr hc; hdr_of(s, hc);
      int offset = in_range(hc, 0, k) ? m_of(hc, k) : WFA_NULL;
      int v = offset - k, h = offset;
      bool broken = false;
      // INS: the insertion run the backtrace is inside of (ins_run characters so far, all to the right of h) becomes a record when the first
      // operation that is no insertion shows where it begins: rp reference sites and sp query characters lie to its left.  One lane takes
      // the slot and stores the record; a record that finds the buffer full is counted and the query is run again with a larger one.
      int ins_run = 0, ins_n = 0;
      bool ins_full = false;
      auto ins_end = [&](int rp, int sp) {
        if constexpr (INS) {
          if (ins_run > 0) {
            unsigned slot = 0;
            if (lane == 0) slot = (unsigned)atomicAdd(ins.n_rec, 1);
            slot = (unsigned)rfl((int)slot);
            if (slot < (unsigned)ins.cap) { if (lane == 0) ins.rec[slot] = make_int4(q, rp, sp, ins_run); }
            else ins_full = true;
            ins_n++; ins_run = 0;
          }
        }
      };
      while (v > 0 && h > 0 && s > 0) {
        if (state == 0) {
          // A run of mismatches on one diagonal with no matches between them (an N run of the query): lane j looks at the cell
          // j mismatches back; the leading lanes whose cell came from a mismatch and was not extended are taken in one go.
          const int sj = s - lane * P.x;
          int cj = -1, mj = WFA_NULL;
          if (sj >= 0) { Hdr hj; hdr_of(sj, hj); if (in_range(hj, 0, k)) { mj = m_of(hj, k); cj = code_of(hj, k) & 7; } }
          const int mnext = __shfl_down(mj, 1);
          const bool pure = lane < 63 && sj > 0 && cj == C_MISMATCH && mnext != WFA_NULL && mj == mnext + 1 && v - lane > 0 && h - lane > 0;
          const unsigned long long np = ~__ballot(pure);
          const int n = np ? __builtin_ctzll(np) : 63;
          if (n > 0) {
            ins_end(v, h);
            if (lane < n && v - 1 - lane <= plen) row[v - 1 - lane] = text[h - 1 - lane];
            s -= n * P.x; offset -= n; v -= n; h -= n;
            continue;
          }
          const int c = __shfl(cj, 0);
          if (c < 0) { broken = true; break; }
          int max_all = WFA_NULL;
          if (c == C_MISMATCH) { const int mn = __shfl(mj, 1); if (mn == WFA_NULL) { broken = true; break; } max_all = mn + 1; }
          else if (c == C_INS_OPEN || c == C_DEL_OPEN) {
            const int ss = s - P.oe, kk = c == C_INS_OPEN ? k - 1 : k + 1;
            Hdr ho; if (ss < 0) { broken = true; break; } hdr_of(ss, ho);
            if (!in_range(ho, 0, kk)) { broken = true; break; }
            max_all = m_of(ho, kk) + (c == C_INS_OPEN ? 1 : 0);
          } else {                                               // a gap being extended: follow it to the M cell it was opened from
            const int dk = c == C_INS_EXT ? -1 : 1, bit = c == C_INS_EXT ? C_I_EXT : C_D_EXT;
            int ss = s - P.e, kk = k + dk, cnt = 0;
            for (;;) {
              Hdr hw; if (ss < 0) { broken = true; break; } hdr_of(ss, hw);
              if (!cell_ok(hw, kk)) { broken = true; break; }
              cnt++;
              if (!(code_of(hw, kk) & bit)) {
                Hdr ho; if (ss - P.oe < 0) { broken = true; break; } hdr_of(ss - P.oe, ho);
                if (!in_range(ho, 0, kk + dk)) { broken = true; break; }
                max_all = m_of(ho, kk + dk) + (c == C_INS_EXT ? cnt + 1 : 0);
                break;
              }
              ss -= P.e; kk += dk;
            }
            if (broken) break;
          }
          const int nm = offset - max_all;
          if (nm < 0 || (nm > 0 && (max_all < 0 || max_all - k < 0 || v > plen + 1 || h > tlen + 1))) { broken = true; break; }   // (a consistent backtrace never gets here)
          bool bad = false;
          if (nm > 0) ins_end(v, h);
          for (int j0 = 0; j0 < nm; j0 += 64) {
            const int j = j0 + lane;
            if (j < nm) { const uint8_t ch = text[h - 1 - j]; if (ch != ref[v - 1 - j]) bad = true; row[v - 1 - j] = ch; }
          }
          if (__any(bad)) { broken = true; break; }
          offset = max_all;
          v = offset - k; h = offset;
          if (c == C_INS_EXT || c == C_INS_OPEN) ins_run++; else ins_end(v, h);
          if (c == C_DEL_EXT)        { if (lane == 0 && v > 0 && v <= plen) row[v - 1] = '-'; s -= P.e;  k++; state = 2; }
          else if (c == C_DEL_OPEN)  { if (lane == 0 && v > 0 && v <= plen) row[v - 1] = '-'; s -= P.oe; k++; state = 0; }
          else if (c == C_INS_EXT)   { s -= P.e;  k--; offset--; state = 1; }
          else if (c == C_INS_OPEN)  { s -= P.oe; k--; offset--; state = 0; }
          else                       { if (lane == 0 && v > 0 && h > 0 && v <= plen + 1) row[v - 1] = text[h - 1]; s -= P.x; offset--; }
        } else {
          Hdr hw; hdr_of(s, hw);
          if (!cell_ok(hw, k)) { broken = true; break; }
          const int cb = code_of(hw, k);
          if (state == 1) { const bool ext = cb & C_I_EXT; ins_run++; s -= ext ? P.e : P.oe; k--; offset--; state = ext ? 1 : 0; }
          else { const bool ext = cb & C_D_EXT; if (lane == 0 && v > 0 && v <= plen) row[v - 1] = '-'; s -= ext ? P.e : P.oe; k++; state = ext ? 2 : 0; }
        }
        v = offset - k; h = offset;
      }
      if (broken || s < 0) status = ST_BACKTRACE;
      else if (s == 0) { for (int j = lane; j < min(v, plen); j += 64) row[j] = text[j]; }      // the last stroke of matches (k = 0 at score 0)
      else { for (int j = lane; j < min(v, plen); j += 64) row[j] = '-'; }                      // leading deletions; leading insertions leave no trace
      if (lane == 0) row[plen] = 0;
      if constexpr (INS) {
        if (status == ST_OK) {
          if (s > 0 && v <= 0 && h > 0) { ins_run += h; h = 0; }             // the leading insertion (the `while (h > 0)` of the oracle's backtrace)
          ins_end(max(v, 0), max(h, 0));
          if (lane == 0) ins.runs[q] = ins_n;
          if (ins_full) status = ST_INSFULL;
        }
      }
    }
    if (tid == 0) {
      score_out[q] = status == ST_OK ? score : -1; status_out[q] = status;     // (thread 0 belongs to the wave that ran the backtrace)
      if (n_own > 0) {                                           // the chunks taken for this query go back
        pool_lock(ctl);
        int top = atomicAdd(&ctl->top, 0);
        for (int i = 0; i < n_own; i++) atomicExch(&stack[top++], own[i]);
        atomicExch(&ctl->top, top);
        pool_unlock(ctl);
      }
    }
    if (status == ST_OK) cells_total += cells;                   // (a query that is run again is counted by the pass that completes it)
    __syncthreads();
  }
  if (tid == 0 && cells_total) atomicAdd(cells_out, cells_total);
