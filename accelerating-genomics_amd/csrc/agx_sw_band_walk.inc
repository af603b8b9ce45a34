// The band-aware walk over a traced banded fill's directions (agx_sw_band_trace_kernel.hip has the contract; DESIGN.md 4.1h):
// the statements of sw_walk_band's body, and with AT of sw_walk_band_at's (agx_sw_band_diag_trace_kernel.hip; DESIGN.md 4.1j),
// whose spans begin inside the resident image: there SwWalkRec.reserved holds the bytes between the record's y_dw and the byte
// in front of the span's first target symbol (the start phase of the fill), and SwBandWalkRec.fpad the bytes in front of its
// first query symbol.  State machine, guards and stores are the same in both builds.
// A fragment, included INSIDE the body of a kernel with the parameters (recs, band, n, img, trace, slots, runs) behind a
// `constexpr bool AT`: as an inlined function template the compiler schedules sw_walk_band differently from the code it had.
// A second `constexpr bool DUAL` (agx_sw_band_dual_trace_kernel.hip; DESIGN.md 4.1o) reads the traced two-piece fill's BYTES: five
// states, H and a gap state per piece and direction, the same guards in front of the one load, the same stores.  Everything it
// adds stands inside `if constexpr`.
    const uint32_t p = blockIdx.x * 64u + threadIdx.x;
    if (p >= n) return;
    const SwWalkRec r = recs[p];
    const SwBandWalkRec bw = band[p];
    const uint32_t G = r.G, ks = bw.kshift, W = DUAL ? (uint32_t)sw_band_dual_trace_words((int)r.C) : (uint32_t)sw_band_trace_words((int)r.C);
    const uint32_t *tr = trace + r.goff;
    const uint8_t *x = reinterpret_cast<const uint8_t *>(img + r.x_dw) + bw.fpad;  // x[j - 1]
    const uint8_t *y = reinterpret_cast<const uint8_t *>(img + r.y_dw) + 1;        // y[i - 1]
    if constexpr (AT) y += r.reserved;
    uint32_t *out = slots + r.slot + ((uint64_t)r.ca + r.cb); // one past the slot's last word
    uint32_t i = r.cb, j = r.ca, n_runs = 0, op = 0, len = 0;
    int state = 0; // 0 H, 1 E, 2 F (DUAL: 1 E1, 2 F1, 3 E2, 4 F2)
    bool failed = false;
    auto emit = [&](uint32_t o, uint32_t k) {
        if (o == op) len += k;
        else {
            if (len) {
                *--out = len << 4 | op;
                ++n_runs;
            }
            op = o;
            len = k;
        }
    };
    while (i || j) {
        const int d = (int)j - (int)i;
        if (d < bw.dlo || d > bw.dhi || i > r.cb || j > r.ca) {
            failed = true;
            break;
        }
        // Row 0 and column 0 are reached in state H (the fill's head comment); the test does not ask the state.  The run along
        // the boundary stays in the band: it ends at diagonal 0.
        if (i == 0) {
            emit(1u, j);
            break;
        }
        if (j == 0) {
            emit(2u, i);
            break;
        }
        const uint32_t slot = (uint32_t)(d - bw.dlo), lane = slot >> ks, k = slot - (lane << ks);
        if (lane >= G) { // (G K >= dhi - dlo + 1 by the plan; a record that says otherwise must not steer a load)
            failed = true;
            break;
        }
        if constexpr (DUAL) {
            const uint32_t cell = tr[((uint64_t)(i + lane) * G + lane) * W + (k >> 2)] >> (8u * (k & 3u)) & 255u;
            if (state == 0) {
                const uint32_t src = cell & 3u;
                if (src == 0u) {
                    emit(x[j - 1u] == y[i - 1u] ? 7u : 8u, 1u);
                    --i;
                    --j;
                } else if (src == 3u) { // (no fill writes it)
                    failed = true;
                    break;
                } else
                    state = (int)src + (cell & 4u ? 2 : 0);
            } else if (state & 1) { // E1 or E2: its own piece's bit
                emit(2u, 1u);
                state = cell & (state == 1 ? 16u : 64u) ? state : 0;
                --i;
            } else {
                emit(1u, 1u);
                state = cell & (state == 2 ? 32u : 128u) ? state : 0;
                --j;
            }
            continue;
        }
        const uint32_t nib = tr[((uint64_t)(i + lane) * G + lane) * W + (k >> 3)] >> (4u * (k & 7u)) & 15u;
        if (state == 0) {
            const uint32_t src = nib & 3u;
            if (src == 0u) {
                emit(x[j - 1u] == y[i - 1u] ? 7u : 8u, 1u);
                --i;
                --j;
            } else
                state = (int)src;
        } else if (state == 1) {
            emit(2u, 1u);
            state = nib & 4u ? 1 : 0;
            --i;
        } else {
            emit(1u, 1u);
            state = nib & 8u ? 2 : 0;
            --j;
        }
    }
    if (len) {
        *--out = len << 4 | op;
        ++n_runs;
    }
    runs[p] = failed ? kSwWalkFailed : n_runs;
