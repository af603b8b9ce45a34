// The walk over a traced fill's directions, and the gather of its runs (agx_sw_batch_cigars; include/agx.h, "Alignment itself";
// DESIGN.md 4.1f).  One lane per traced pair: from the corner (cb, ca) in state H it follows the four bits the traced fill
// (agx_sw_anch_kernel.inc, TRACE) left per cell -- row i, column j (0-based) at lane j / C, nibble j % C, step i + j / C -- a
// chain of about ca + cb dependent loads.  State H reads where H came from (diagonal: '=' where the symbols of the image
// agree, else 'X'; E; F), state E emits D and stays while bit 2 says E extended, state F emits I and stays on bit 3; row 0
// and column 0 are reached in state H only and end the walk with one run.  Runs are merged as they are made and written from
// the end of the pair's slot of ca + cb words backwards, so that they read forwards.
#include "agx_sw.h"

namespace {

__global__ void __launch_bounds__(64) sw_walk(const SwWalkRec *__restrict__ recs, uint32_t n, const uint32_t *__restrict__ img,
                                              const uint32_t *__restrict__ trace, uint32_t *__restrict__ slots, uint32_t *__restrict__ runs)
{
    const uint32_t p = blockIdx.x * 64u + threadIdx.x;
    if (p >= n) return;
    const SwWalkRec r = recs[p];
    const uint32_t G = r.G, C = r.C, W = (uint32_t)sw_trace_words((int)r.C);
    const uint32_t *tr = trace + r.goff;
    const uint8_t *x = reinterpret_cast<const uint8_t *>(img + r.x_dw), *y = reinterpret_cast<const uint8_t *>(img + r.y_dw);
    uint32_t *out = slots + r.slot + ((uint64_t)r.ca + r.cb); // one past the slot's last word
    uint32_t i = r.cb, j = r.ca, n_runs = 0, op = 0, len = 0;
    int state = 0; // 0 H, 1 E, 2 F
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
        // Row 0 and column 0 are reached in state H: the traced fill never sets "E extended" in row 1 nor "F extended" in column
        // 1.  The test does not ask the state, so that no word of the block, whatever it holds, can lead a load out of it.
        if (i == 0) {
            emit(1u, j);
            break;
        }
        if (j == 0) {
            emit(2u, i);
            break;
        }
        const uint32_t row = i - 1u, col = j - 1u, lane = col / C, k = col - lane * C;
        const uint32_t nib = tr[((uint64_t)(row + lane) * G + lane) * W + (k >> 3)] >> (4u * (k & 7u)) & 15u;
        if (state == 0) {
            const uint32_t src = nib & 3u;
            if (src == 0u) {
                emit(x[col] == y[row] ? 7u : 8u, 1u);
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
    runs[p] = n_runs;
}

// one wavefront per pair: its runs, right-aligned in its slot, to out + dst[pair]
__global__ void __launch_bounds__(256) sw_gather(const SwWalkRec *__restrict__ recs, uint32_t n, const uint32_t *__restrict__ slots,
                                                 const uint32_t *__restrict__ runs, const uint64_t *__restrict__ dst, uint32_t *__restrict__ out)
{
    const uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (p >= n) return;
    const uint32_t cnt = runs[p];
    const uint32_t *src = slots + recs[p].slot + ((uint64_t)recs[p].ca + recs[p].cb - cnt);
    uint32_t *to = out + dst[p];
    for (uint32_t k = threadIdx.x & 63u; k < cnt; k += 64u) to[k] = src[k];
}

} // namespace

int agx_sw_walk_launch(const SwWalkRec *recs, uint32_t n, const uint32_t *img, const uint32_t *trace, uint32_t *slots, uint32_t *runs, hipStream_t s)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(sw_walk, dim3((n + 63u) / 64u), dim3(64), 0, s, recs, n, img, trace, slots, runs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int agx_sw_gather_launch(const SwWalkRec *recs, uint32_t n, const uint32_t *slots, const uint32_t *runs, const uint64_t *dst, uint32_t *out,
                         hipStream_t s)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(sw_gather, dim3((n + 3u) / 4u), dim3(256), 0, s, recs, n, slots, runs, dst, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void agx_sw_walk_preload()
{
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&sw_walk));
}
