// gj_dec_entropy_prog_body.h -- the body of k_huffman_decode_prog and k_huffman_decode_prog_batch (gj_dec_entropy_prog.hip), included once in each:
// the single-frame kernel is then, statement for statement, the code it has always been (its schedule is measured: profiles/progressive.md), and the
// batched kernel cannot drift from it. What the including kernel provides: blockIdx.x < rec_count; `recs`; the stream [jpeg, jpeg + jpeg_size) the
// record's pos / len are clamped to; `tabs`, `tab_count` and GJ_PROG_TABLE(t), the pool entry of the record's table number t (clamped to the pool
// here); the planes [coefs, coefs + 64 coef_blocks) the record's block numbers are clamped to.
    __shared__ uint16_t s_tab[GJ_MAX_COMP * GJ_DEC_TAB_WORDS];
    __shared__ uint32_t s_stage[GJ_PROG_STAGE_DW];
    __shared__ uint8_t s_zz[64];
    __shared__ uint16_t s_ahead[GJ_PROG_AHEAD * 64];
    const int lane = threadIdx.x;
    s_zz[lane] = GJ_ZZ[lane];
    __syncthreads();
    const gj_prog_rec& R = recs[blockIdx.x]; // (an address that is the same in every lane: scalar loads)
    const int kind = R.kind;
    const int ncomp = min(max((int)R.ncomp, 1), GJ_MAX_COMP);
    const bool uses_tables = kind != GJ_PROG_DC_REFINE;
    for (int c = 0; uses_tables && c < ncomp; c++) { // the tables of the segment's scan: one per component of a first DC scan, one of an AC scan
        static_assert(GJ_DEC_TAB_WORDS % 2 == 0, "tables are copied as dwords");
        const uint32_t* from = reinterpret_cast<const uint32_t*>(tabs + (size_t)min(GJ_PROG_TABLE(R.c[c].table), max(tab_count, 1u) - 1u) * GJ_DEC_TAB_WORDS);
        for (int t = lane; t < GJ_DEC_TAB_WORDS / 2; t += 64) reinterpret_cast<uint32_t*>(s_tab + c * GJ_DEC_TAB_WORDS)[t] = tab_count ? from[t] : 0u;
    }
    __syncthreads();

    GjProgBits B;
    {
        const uint32_t pos = R.pos <= jpeg_size ? R.pos : (uint32_t)jpeg_size;
        B.len = (uint64_t)R.len <= jpeg_size - pos ? R.len : (uint32_t)(jpeg_size - pos);
        const uintptr_t a = reinterpret_cast<uintptr_t>(jpeg) + pos;
        B.src = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
        B.end = reinterpret_cast<const uint32_t*>((reinterpret_cast<uintptr_t>(jpeg) + jpeg_size + 3) & ~(uintptr_t)3);
        B.lead = (int)(a & 3);
        B.ndw = ((uint32_t)B.lead + B.len + 3u) >> 2;
        B.c0 = 0;
        B.carry = 0;
        B.sbytes = 0;
        B.bitpos = 0;
        B.acc = 0;
        B.n = 0;
    }
    uint32_t per_mcu = 0;
    for (int c = 0; c < ncomp; c++) per_mcu += (uint32_t)R.c[c].h * R.c[c].v;
    per_mcu = max(per_mcu, 1u);
    const uint32_t total = R.count * per_mcu; // blocks of the segment
    const int al = min((int)R.al, 13);
    const int ss = min((int)R.ss, 63), se = min((int)R.se, 63);

    if (kind == GJ_PROG_DC_FIRST) {
        int pred[GJ_MAX_COMP] = {0, 0, 0, 0};
        int my_val = 0;
        uint32_t my_blk = 0;
        for (uint32_t o = 0; o < total; o++) {
            gj_prog_need(B, s_stage, lane);
            int ci;
            const uint32_t blk = gj_prog_block(R, per_mcu, o, ci);
            const uint32_t sz = gj_prog_symbol(B, s_stage, s_tab + ci * GJ_DEC_TAB_WORDS) & 15u;
            const uint32_t bits = gj_prog_get(B, s_stage, sz);
            const int diff = (sz && bits < (1u << (sz - 1))) ? (int)bits - (int)((1u << sz) - 1u) : (int)bits;
            const int v = (ci == 0 ? pred[0] : ci == 1 ? pred[1] : ci == 2 ? pred[2] : pred[3]) + diff;
            if (ci == 0) pred[0] = v; else if (ci == 1) pred[1] = v; else if (ci == 2) pred[2] = v; else pred[3] = v;
            if (lane == (int)(o & 63u)) { my_val = v * (1 << al); my_blk = blk; }
            if ((o & 63u) == 63u || o + 1u == total) { // 64 blocks at a time
                if ((uint32_t)lane <= (o & 63u) && my_blk < coef_blocks) coefs[(uint64_t)my_blk * 64] = (int16_t)my_val;
            }
        }
    } else if (kind == GJ_PROG_DC_REFINE) {
        for (uint32_t o = 0; o < total; o += 64u) {
            gj_prog_need(B, s_stage, lane);
            const uint32_t n = min(total - o, 64u);
            if ((uint32_t)lane < n) {
                int ci;
                const uint32_t blk = gj_prog_block(R, per_mcu, o + (uint32_t)lane, ci);
                if (gj_prog_bit(B, s_stage, B.bitpos + (uint32_t)lane) && blk < coef_blocks) {
                    int16_t* p = coefs + (uint64_t)blk * 64;
                    *p = (int16_t)(*p | (1 << al));
                }
            }
            B.bitpos += n; // (this kind of scan reads single bits of the stage: the window is not used)
        }
    } else {
        const gj_prog_comp& K = R.c[0];
        const uint16_t* tac = s_tab;
        const bool in_band = lane >= ss && lane <= se;
        const unsigned long long band = ((se >= 63 ? ~0ull : ((1ull << (se + 1)) - 1ull)) >> ss) << ss;
        const int p1 = 1 << al, m1 = -(1 << al);
        uint32_t eobrun = 0;
        for (uint32_t o = 0; o < total; o++) {
            if (kind == GJ_PROG_AC_FIRST && eobrun > 0) { // whole blocks without a coefficient of this band
                const uint32_t skip = min(eobrun, total - o);
                eobrun -= skip;
                o += skip - 1u;
                continue;
            }
            const uint32_t m = R.first + o;
            const uint32_t by = m / R.across, bx = m - by * R.across;
            const uint64_t blk = (uint64_t)K.base + (uint64_t)by * K.pitch + bx;
            const bool inside = blk < coef_blocks;
            int16_t* mine = coefs + (inside ? blk : 0) * 64 + s_zz[lane];
            if (kind == GJ_PROG_AC_FIRST) {
                int val = 0;
                int k = ss;
                while (k <= se) {
                    gj_prog_need(B, s_stage, lane);
                    const uint32_t sym = gj_prog_symbol(B, s_stage, tac);
                    const int r = (int)(sym >> 4), s = (int)(sym & 15u);
                    if (s) {
                        k += r;
                        const uint32_t bits = gj_prog_get(B, s_stage, (uint32_t)s);
                        const int v = bits < (1u << (s - 1)) ? (int)bits - (int)((1u << s) - 1u) : (int)bits;
                        if (lane == min(k, 63) && k <= se) val = v * (1 << al);
                        k++;
                    } else if (r == 15) {
                        k += 16;
                    } else {
                        eobrun = (1u << r) + gj_prog_get(B, s_stage, (uint32_t)r) - 1u; // this block ends here, eobrun more follow
                        eobrun = min(eobrun, total - o - 1u);
                        break;
                    }
                }
                if (in_band && val != 0 && inside) *mine = (int16_t)val;
            } else {
                // The lanes load the block -- but not when its turn comes: a lone wave would wait for a trip to memory per block (behind its own
                // stores of the block before: loads and stores share one counter), 2.7 us a block where the decode takes a tenth of that. Every
                // GJ_PROG_AHEAD blocks the lanes load their coefficient of ALL of them, the loads in flight together, and park them in LDS; no scan
                // of this launch writes them (this wave alone owns these coefficients, and a block is changed only in its own turn).
                if ((o & (GJ_PROG_AHEAD - 1u)) == 0u) {
                    uint16_t ahead[GJ_PROG_AHEAD];
#pragma unroll
                    for (uint32_t a = 0; a < GJ_PROG_AHEAD; a++) {
                        const uint32_t ma = R.first + o + a;
                        const uint32_t ya = ma / R.across, xa = ma - ya * R.across;
                        const uint64_t ba = (uint64_t)K.base + (uint64_t)ya * K.pitch + xa;
                        ahead[a] = in_band && o + a < total && ba < coef_blocks ? (uint16_t)coefs[ba * 64 + s_zz[lane]] : (uint16_t)0;
                    }
                    gj_wave_sync();
#pragma unroll
                    for (uint32_t a = 0; a < GJ_PROG_AHEAD; a++) s_ahead[a * 64u + (uint32_t)lane] = ahead[a];
                    gj_wave_sync();
                }
                int c = (int16_t)s_ahead[(o & (GJ_PROG_AHEAD - 1u)) * 64u + (uint32_t)lane];
                const int before = c;
                const unsigned long long hist = __ballot(c != 0) & band;
                int k = ss;
                if (eobrun == 0) {
                    while (k <= se) {
                        gj_prog_need(B, s_stage, lane);
                        const uint32_t sym = gj_prog_symbol(B, s_stage, tac);
                        const int r = (int)(sym >> 4), s = (int)(sym & 15u);
                        int newval = 0;
                        if (s) {
                            newval = gj_prog_get(B, s_stage, 1u) ? p1 : m1;
                        } else if (r != 15) {
                            eobrun = (1u << r) + gj_prog_get(B, s_stage, (uint32_t)r); // this block included
                            break;
                        }
                        // the stretch [k, t): t = the (r + 1)-th coefficient without history from k on, or the end of the band
                        const unsigned long long from_k = ~0ull << k;
                        unsigned long long z = ~hist & band & from_k;
                        for (int i = 0; i < r && z; i++) z &= z - 1ull;
                        const int t = z ? __builtin_ctzll(z) : se + 1;
                        const unsigned long long stretch = hist & from_k & (t >= 64 ? ~0ull : ((1ull << t) - 1ull));
                        if ((stretch >> lane) & 1ull) { // my correction bit: as many bits in front of it as corrected coefficients in front of me
                            const uint32_t rank = (uint32_t)__popcll(stretch & ((1ull << lane) - 1ull));
                            if (gj_prog_bit(B, s_stage, B.bitpos + rank) && (c & p1) == 0) c += c >= 0 ? p1 : m1;
                        }
                        gj_prog_skip(B, s_stage, (uint32_t)__popcll(stretch));
                        if (s && t <= se && lane == t) c = newval;
                        k = t + 1;
                    }
                }
                if (eobrun > 0) { // the rest of the band: correction bits only
                    gj_prog_need(B, s_stage, lane);
                    const unsigned long long stretch = k <= se ? hist & (~0ull << k) : 0ull;
                    if ((stretch >> lane) & 1ull) {
                        const uint32_t rank = (uint32_t)__popcll(stretch & ((1ull << lane) - 1ull));
                        if (gj_prog_bit(B, s_stage, B.bitpos + rank) && (c & p1) == 0) c += c >= 0 ? p1 : m1;
                    }
                    gj_prog_skip(B, s_stage, (uint32_t)__popcll(stretch));
                    eobrun--;
                }
                if (in_band && inside && c != before) *mine = (int16_t)c;
            }
        }
    }
