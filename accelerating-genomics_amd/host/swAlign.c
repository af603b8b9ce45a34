/*
 * swAlign <file_path> [local|global|fit|extend|extend-query]: where the best alignment of every pair ends and begins
 * (default: local; the other modes are include/agx.h's "Alignment modes").
 * Reads the Smith-Waterman input format of `antidiagonalSmithWaterman` (header = number of sequence lines, pair p =
 * lines 2p and 2p+1, the newline kept as a symbol) through agx_sw_reader_* and prints one line per pair, in file order:
 *     score a_begin a_end b_begin b_end
 * a = the pair's first line (the query), b = its second (the target); positions are 0-based and inclusive, all -1 when
 * the score is 0 (include/agx.h, "Alignment coordinates").  The fill and the begin pass run on GPU 0 through libagx;
 * there is no CPU path.
 *   AGX_CLI_CHUNK_PAIRS   pairs per agx_sw_align call (default 262144)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "agx.h"

int main(int argc, char *argv[])
{
    static const char *const words[] = {"local", "global", "fit", "extend", "extend-query"}; /* AGX_SW_MODE_* 0..4 */
    int mode = argc == 2 ? AGX_SW_MODE_LOCAL : -1;
    for (int k = 0; argc == 3 && k < 5; k++)
        if (!strcmp(argv[2], words[k])) mode = k;
    if (mode < 0) {
        fprintf(stderr, "Usage: %s <file_path> [local|global|fit|extend|extend-query]\n", argv[0]);
        return 1;
    }
    const char *cp = getenv("AGX_CLI_CHUNK_PAIRS");
    const int64_t chunk_pairs = cp && atoll(cp) > 0 ? atoll(cp) : 262144;
    agx_sw_reader *reader = NULL;
    if (agx_sw_reader_open(argv[1], 0, &reader) != AGX_OK) {
        fprintf(stderr, "swAlign: %s\n", agx_last_error());
        return EXIT_FAILURE;
    }
    agx_ctx *ctx = NULL;
    int status = 0;
    while (!status && !agx_sw_reader_done(reader)) {
        agx_sw_text *t = NULL;
        if (agx_sw_reader_next(reader, chunk_pairs, &t) != AGX_OK) {
            fprintf(stderr, "swAlign: %s\n", agx_last_error());
            status = EXIT_FAILURE;
            break;
        }
        if (t->n_pairs > 0) {
            agx_sw_hit *hits = (agx_sw_hit *)malloc(sizeof(agx_sw_hit) * (size_t)t->n_pairs);
            if (!hits) {
                fprintf(stderr, "swAlign: out of memory\n");
                status = EXIT_FAILURE;
            }
            if (!status && !ctx && agx_ctx_create(0, &ctx) != AGX_OK) {
                fprintf(stderr, "swAlign: %s\n", agx_last_error());
                status = EXIT_FAILURE;
            }
            if (!status && agx_sw_align_mode(ctx, NULL, mode, AGX_SW_ALIGN_SPANS, t->bases, t->off, t->len, t->n_pairs, hits) != AGX_OK) {
                fprintf(stderr, "swAlign: %s\n", agx_last_error());
                status = EXIT_FAILURE;
            }
            if (!status)
                for (int64_t p = 0; p < t->n_pairs; p++)
                    printf("%d %d %d %d %d\n", hits[p].score, hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end);
            free(hits);
        }
        agx_sw_text_free(t);
    }
    agx_sw_reader_close(reader);
    if (ctx) agx_ctx_destroy(ctx);
    return status;
}
