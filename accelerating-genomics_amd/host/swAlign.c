/*
 * swAlign <file_path> [local|global|fit|extend|extend-query][+stats|+cigar|+band=W|+cigar+band=W|+band=W@D|+bandcigar=W@D|+bandstats=W@D][+zdrop=Z]
 * (and, with a matrix file, +matband=W@D|+matbandcigar=W@D; with six scoring numbers, +dualband=W@D|+dualbandcigar=W@D): where the best alignment of every pair ends and begins
 * (default: local; the other modes are include/agx.h's "Alignment modes").
 * swAlign <file_path> <mode> <matrix_file> [gap_open gap_extend]: the same under a substitution matrix (gaps default to
 * -11 -1).  The matrix file is the usual text layout: '#' comment lines, one line of symbols, then one row per symbol
 * holding the symbol followed by its integers; at most 32 symbols, letters in either case, the matrix symmetric.  With a
 * matrix the trailing "\n" or "\r\n" of every line is stripped before aligning: a newline is not a residue.
 * Reads the Smith-Waterman input format of `antidiagonalSmithWaterman` (header = number of sequence lines, pair p =
 * lines 2p and 2p+1, the newline kept as a symbol) through agx_sw_reader_* and prints one line per pair, in file order:
 *     score a_begin a_end b_begin b_end
 * a = the pair's first line (the query), b = its second (the target); positions are 0-based and inclusive, all -1 when
 * the score is 0 (include/agx.h, "Alignment coordinates").  The fill and the begin pass run on GPU 0 through libagx;
 * there is no CPU path.
 * The mode word may carry the suffix "+stats" (local+stats, fit+stats ...): every line then ends in two more numbers,
 *     score a_begin a_end b_begin b_end matches pairs
 * the identical symbols and the aligned pairs of that alignment (include/agx.h, "Alignment statistics"; queries up to
 * AGX_SW_STATS_MAX_QUERY_LEN).  Without the suffix the output is what it was.
 * Or the suffix "+cigar" (local+cigar, fit+cigar ...), with or without a matrix file: every line then ends in the alignment,
 *     score a_begin a_end b_begin b_end CIGAR
 * as text with '=', 'X', 'I' and 'D' over the span the line names, "*" for an alignment that consumes nothing (include/agx.h,
 * "Alignment itself"; queries up to AGX_SW_CIGAR_MAX_QUERY_LEN).  "+stats+cigar" is not offered.
 * Or the suffix "+band=W" on global and extend (global+band=64, extend+band=200): the BANDED alignment of half-width W
 * (include/agx.h, "Banded alignment"), for long similar pairs -- both sides up to AGX_SW_BAND_MAX_LEN symbols.  The lines are
 *     score a_begin a_end b_begin b_end
 * and the input is read with a line buffer of 65 536 bytes, so lines of up to 65 535 bytes stay whole (without the suffix the
 * reader keeps the reference's 1 000).  Not with another mode, not together with +stats or a matrix file.
 * Or "+cigar+band=W" on global and extend, in this order (global+cigar+band=64): the banded alignment and its CIGAR inside the
 * band (include/agx.h, "CIGARs for banded batches"), the lines of "+cigar" read with the line buffer of "+band=W".
 * "global+band=3+cigar" is a usage error.
 * Or the suffix "+band=W@D" on any mode (fit+band=64@0, local+band=200@-1500, extend-query+band=32@0): the alignment inside the
 * band D - W <= j - i <= D + W around the diagonal D, one signed number for every pair of the file (include/agx.h, "Banded
 * alignment around a diagonal"); the lines of "+band=W", read with its line buffer.  Not together with +stats, +cigar or a
 * matrix file: "global+cigar+band=8@0" is a usage error.  Without "@D" nothing changes: "global+band=64" is the banded
 * alignment of "Banded alignment", "fit+band=3" a usage error.
 * Or the suffix "+bandcigar=W@D" on any mode (fit+bandcigar=64@-1500, local+bandcigar=200@0): the alignment inside the band
 * around the diagonal D AND its CIGAR inside that band (include/agx.h, "CIGARs for batches banded around a diagonal"): the lines
 * of "+band=W@D" with the CIGAR text appended as "+cigar" formats it, read with the line buffer of "+band=W".  W and D as in
 * "+band=W@D", both required; no matrix file.
 * Or "+zdrop=Z" behind either of the last two on extend, in this place only (extend+band=64@0+zdrop=100,
 * extend+bandcigar=64@0+zdrop=100): the extension terminates by the z-drop Z >= 0 (include/agx.h, "Z-drop for banded extension");
 * the same lines as without the suffix.  Another mode, a negative or non-numeric Z, or the suffix anywhere else is a usage error.
 * Or the suffix "+bandstats=W@D" on any mode (fit+bandstats=64@-1500, global+bandstats=128@0): the alignment inside the band around
 * the diagonal D AND its matches and aligned pairs, with no traceback (include/agx.h, "Statistics for batches banded around a
 * diagonal"): the lines of "+band=W@D" with the two numbers appended as "+stats" appends them, read with the line buffer of
 * "+band=W".  W and D as in "+band=W@D", both required; no matrix file, and no +cigar or +zdrop behind it.
 * swAlign <file_path> <mode>+matband=W@D <matrix_file> [gap_open gap_extend]: the lines of "+band=W@D" under the substitution
 * matrix (include/agx.h, "Banded alignment around a diagonal under a substitution matrix"), and
 * swAlign <file_path> <mode>+matbandcigar=W@D <matrix_file> [gap_open gap_extend]: the lines of "+bandcigar=W@D" under it.  Any
 * mode; W and D as in "+band=W@D", both required; read with the line buffer of "+band=W", the line ends stripped as with every
 * matrix file.  Either word without a matrix file, or with +stats, +cigar or +zdrop, is a usage error; so is a matrix file behind
 * "+band=W@D" or "+bandcigar=W@D".
 * swAlign <file_path> <mode>+dualband=W@D <match> <mismatch> <gap_open> <gap_extend> <gap_open2> <gap_extend2>: the lines of
 * "+band=W@D" under two-piece gap costs -- a gap of L symbols scores max(gap_open + L gap_extend, gap_open2 + L gap_extend2), as in
 * minimap2's -O4,24 -E2,1 (include/agx.h, "Banded alignment around a diagonal under two-piece gap costs").  Any mode; W and D as in
 * "+band=W@D", both required; read with the line buffer of "+band=W".  All six numbers are required and must be integers: any
 * other count of arguments, a number that is not one, or a further suffix (+stats, +cigar, +zdrop) is a usage error.
 * swAlign <file_path> <mode>+dualbandcigar=W@D <match> <mismatch> <gap_open> <gap_extend> <gap_open2> <gap_extend2>: the lines of
 * "+dualband=W@D" with the CIGAR inside that band appended as "+bandcigar=W@D" formats it (include/agx.h, "CIGARs for batches
 * banded around a diagonal under two-piece gap costs").  The same rules: all six integers, no further suffix.
 *   AGX_CLI_CHUNK_PAIRS   pairs per agx_sw_align call (default 262144)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <ctype.h>

#include "agx.h"

/* Reads a substitution matrix in the usual text layout into m (gaps are the caller's).  Returns 0, or -1 with a message in err. */
static int read_matrix(const char *path, agx_sw_matrix *m, char *err, size_t err_len)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        snprintf(err, err_len, "cannot open matrix file %s", path);
        return -1;
    }
    char line[4096];
    int n = 0, rows = 0, line_no = 0, rc = 0;
    unsigned char seen[AGX_SW_MATRIX_MAX_SYMBOLS] = {0};
    memset(m->code, 0xff, sizeof m->code);
    memset(m->score, 0, sizeof m->score);
    while (!rc && fgets(line, sizeof line, f)) {
        line_no++;
        char *p = line;
        while (isspace((unsigned char)*p)) p++;
        if (*p == '#' || *p == 0) continue;
        if (n == 0) { /* the line of symbols: single characters separated by blanks */
            while (*p && !rc) {
                if (p[1] && !isspace((unsigned char)p[1])) {
                    snprintf(err, err_len, "%s:%d: the line of symbols holds a word of more than one character", path, line_no);
                    rc = -1;
                } else if (n == AGX_SW_MATRIX_MAX_SYMBOLS) {
                    snprintf(err, err_len, "%s:%d: more than %d symbols", path, line_no, AGX_SW_MATRIX_MAX_SYMBOLS);
                    rc = -1;
                } else if (m->code[(unsigned char)*p] != 0xff) {
                    snprintf(err, err_len, "%s:%d: symbol '%c' appears twice", path, line_no, *p);
                    rc = -1;
                } else {
                    m->code[tolower((unsigned char)*p)] = m->code[toupper((unsigned char)*p)] = (uint8_t)n;
                    n++;
                    p++;
                    while (isspace((unsigned char)*p)) p++;
                }
            }
            continue;
        }
        /* a row: its symbol, then n integers */
        const int a = (p[1] == 0 || isspace((unsigned char)p[1])) ? m->code[(unsigned char)*p] : 0xff;
        if (a == 0xff || seen[a]) {
            snprintf(err, err_len, "%s:%d: the row does not begin with a symbol of the first line that has no row yet", path, line_no);
            rc = -1;
            break;
        }
        seen[a] = 1;
        rows++;
        p++;
        for (int c = 0; c < n && !rc; c++) {
            char *end;
            const long v = strtol(p, &end, 10);
            if (end == p || v < -128 || v > 127) {
                snprintf(err, err_len, "%s:%d: row '%c' needs %d integers in -128..127", path, line_no, line[0], n);
                rc = -1;
            }
            m->score[a][c] = (int8_t)v;
            p = end;
        }
        while (!rc && isspace((unsigned char)*p)) p++;
        if (!rc && *p) {
            snprintf(err, err_len, "%s:%d: more than %d entries in the row", path, line_no, n);
            rc = -1;
        }
    }
    fclose(f);
    if (!rc && (n == 0 || rows != n)) {
        snprintf(err, err_len, "%s: %d symbols but %d rows", path, n, rows);
        rc = -1;
    }
    for (int a = 0; !rc && a < n; a++)
        for (int c = 0; !rc && c < a; c++)
            if (m->score[a][c] != m->score[c][a]) {
                snprintf(err, err_len, "%s: the matrix is not symmetric at (%d, %d): %d against %d", path, a, c, m->score[a][c], m->score[c][a]);
                rc = -1;
            }
    m->n_symbols = n;
    return rc;
}

int main(int argc, char *argv[])
{
    static const char *const words[] = {"local", "global", "fit", "extend", "extend-query"}; /* AGX_SW_MODE_* 0..4 */
    int mode = argc == 2 ? AGX_SW_MODE_LOCAL : -1;
    int with_stats = 0, with_cigar = 0, with_band = 0, with_diag = 0, with_zdrop = 0, with_matband = 0, with_dual = 0;
    int32_t band = 0, diag = 0, zdrop = 0;
    agx_sw_scoring_dual dual = {0, 0, 0, 0, 0, 0};
    for (int k = 0; (argc == 3 || argc == 4 || argc == 6 || argc == 9) && k < 5; k++) {
        const size_t n = strlen(words[k]);
        if (argc == 9) { /* six numbers behind the mode word: "+dualband=W@D" or "+dualbandcigar=W@D" and nothing else */
            if (strncmp(argv[2], words[k], n)) continue;
            const int dual_cigar = !strncmp(argv[2] + n, "+dualbandcigar=", 15);
            if (!dual_cigar && strncmp(argv[2] + n, "+dualband=", 10)) continue;
            /* W@D as for "+band=W@D", up to the end of the word (no further suffix); any mode; every number a whole integer */
            const char *w = argv[2] + n + (dual_cigar ? 15 : 10);
            char *end, *end2;
            const long v = strtol(w, &end, 10);
            if (!isdigit((unsigned char)*w) || *end != '@' || v > 0x7fffffffL) continue;
            const char *d = end + 1;
            const long c = strtol(d, &end2, 10);
            if (!isdigit((unsigned char)d[*d == '-']) || *end2 || c < -0x7fffffffL || c > 0x7fffffffL) continue;
            int32_t *const six[6] = {&dual.match, &dual.mismatch, &dual.gap_open, &dual.gap_extend, &dual.gap_open2, &dual.gap_extend2};
            int good = 1;
            for (int a = 0; a < 6; a++) {
                char *e;
                const long x = strtol(argv[3 + a], &e, 10);
                if (e == argv[3 + a] || *e || x < -0x7fffffffL || x > 0x7fffffffL) good = 0;
                *six[a] = (int32_t)x;
            }
            if (!good) continue;
            mode = k;
            with_band = with_diag = with_dual = 1;
            with_cigar = dual_cigar;
            band = (int32_t)v;
            diag = (int32_t)c;
            continue;
        }
        if (!strcmp(argv[2], words[k])) mode = k;
        const int cigar_band = !strncmp(argv[2], words[k], n) && !strncmp(argv[2] + n, "+cigar+band=", 12); /* in this order only */
        if (!strncmp(argv[2], words[k], n) && (cigar_band || !strncmp(argv[2] + n, "+band=", 6))) {
            /* W: digits only, up to the end of the word; global and extend only, and no matrix file */
            const char *w = argv[2] + n + (cigar_band ? 12 : 6);
            char *end;
            const long v = strtol(w, &end, 10);
            if (isdigit((unsigned char)*w) && !*end && v <= 0x7fffffffL && argc == 3 && (k == AGX_SW_MODE_GLOBAL || k == AGX_SW_MODE_EXTEND)) {
                mode = k;
                with_band = 1;
                with_cigar = cigar_band;
                band = (int32_t)v;
            }
        }
        const int band_cigar = !strncmp(argv[2], words[k], n) && !strncmp(argv[2] + n, "+bandcigar=", 11); /* W@D only */
        if (!strncmp(argv[2], words[k], n) && (band_cigar || !strncmp(argv[2] + n, "+band=", 6)) && argc == 3) {
            /* W@D: digits, '@', an optional '-' and digits, up to the end of the word; any mode, no matrix file */
            const char *w = argv[2] + n + (band_cigar ? 11 : 6);
            char *end, *end2;
            const long v = strtol(w, &end, 10);
            if (isdigit((unsigned char)*w) && *end == '@' && v <= 0x7fffffffL) {
                const char *d = end + 1;
                const long c = strtol(d, &end2, 10);
                /* "+zdrop=Z" may follow on extend: digits only, up to the end of the word */
                long z = -1;
                if (k == AGX_SW_MODE_EXTEND && !strncmp(end2, "+zdrop=", 7) && isdigit((unsigned char)end2[7])) {
                    char *end3;
                    z = strtol(end2 + 7, &end3, 10);
                    if (*end3 || z > 0x7fffffffL) z = -1;
                    else end2 = end3;
                }
                if (isdigit((unsigned char)d[*d == '-']) && !*end2 && c >= -0x7fffffffL && c <= 0x7fffffffL) {
                    mode = k;
                    with_band = with_diag = 1;
                    with_zdrop = z >= 0;
                    zdrop = (int32_t)(z >= 0 ? z : 0);
                    with_cigar = band_cigar;
                    band = (int32_t)v;
                    diag = (int32_t)c;
                }
            }
        }
        if (!strncmp(argv[2], words[k], n) && !strncmp(argv[2] + n, "+bandstats=", 11) && argc == 3) {
            /* W@D as above, up to the end of the word (no further suffix); any mode, no matrix file */
            const char *w = argv[2] + n + 11;
            char *end, *end2;
            const long v = strtol(w, &end, 10);
            if (isdigit((unsigned char)*w) && *end == '@' && v <= 0x7fffffffL) {
                const char *d = end + 1;
                const long c = strtol(d, &end2, 10);
                if (isdigit((unsigned char)d[*d == '-']) && !*end2 && c >= -0x7fffffffL && c <= 0x7fffffffL) {
                    mode = k;
                    with_band = with_diag = with_stats = 1;
                    band = (int32_t)v;
                    diag = (int32_t)c;
                }
            }
        }
        const int mat_cigar = !strncmp(argv[2], words[k], n) && !strncmp(argv[2] + n, "+matbandcigar=", 14);
        if (!strncmp(argv[2], words[k], n) && (mat_cigar || !strncmp(argv[2] + n, "+matband=", 9)) && (argc == 4 || argc == 6)) {
            /* W@D as above, up to the end of the word (no further suffix); any mode, and only with a matrix file */
            const char *w = argv[2] + n + (mat_cigar ? 14 : 9);
            char *end, *end2;
            const long v = strtol(w, &end, 10);
            if (isdigit((unsigned char)*w) && *end == '@' && v <= 0x7fffffffL) {
                const char *d = end + 1;
                const long c = strtol(d, &end2, 10);
                if (isdigit((unsigned char)d[*d == '-']) && !*end2 && c >= -0x7fffffffL && c <= 0x7fffffffL) {
                    mode = k;
                    with_band = with_diag = with_matband = 1;
                    with_cigar = mat_cigar;
                    band = (int32_t)v;
                    diag = (int32_t)c;
                }
            }
        }
        if (!strncmp(argv[2], words[k], n) && !strcmp(argv[2] + n, "+stats")) {
            mode = k;
            with_stats = 1;
        }
        if (!strncmp(argv[2], words[k], n) && !strcmp(argv[2] + n, "+cigar")) {
            mode = k;
            with_cigar = 1;
        }
    }
    if (mode < 0) {
        fprintf(stderr,
                "Usage: %s <file_path> [local|global|fit|extend|extend-query]\n"
                "       %s <file_path> <mode> <matrix_file> [gap_open gap_extend]\n"
                "With a matrix file ('#' comments, a line of symbols, a row per symbol: the symbol and its integers; symmetric,\n"
                "letters in either case) gaps default to -11 -1 and the line ends (\\n, \\r\\n) are stripped, not aligned.\n"
                "<mode>+stats (local+stats, fit+stats ...): every line ends in two more numbers, matches and aligned pairs.\n"
                "<mode>+cigar (local+cigar, fit+cigar ...): every line ends in the alignment as CIGAR text (=, X, I, D; * for none).\n"
                "global+band=W, extend+band=W: the banded alignment of half-width W >= 0 for long pairs (lines of up to 65535 bytes);\n"
                "not with another mode, +stats or a matrix file.\n"
                "global+cigar+band=W, extend+cigar+band=W: the banded alignment with its CIGAR inside the band (in this order).\n"
                "<mode>+band=W@D (fit+band=64@0, local+band=200@-1500): the alignment inside the band D-W <= j-i <= D+W around the\n"
                "diagonal D, in any mode; not with +stats, +cigar or a matrix file.\n"
                "<mode>+bandcigar=W@D (fit+bandcigar=64@-1500): the same with its CIGAR inside that band appended; no matrix file.\n"
                "extend+band=W@D+zdrop=Z, extend+bandcigar=W@D+zdrop=Z: the extension terminates by the z-drop Z >= 0; extend only.\n"
                "<mode>+bandstats=W@D (fit+bandstats=64@-1500): the lines of +band=W@D with matches and aligned pairs appended, no\n"
                "traceback; no matrix file, +cigar or +zdrop.\n"
                "<mode>+matband=W@D <matrix_file> [gap_open gap_extend], <mode>+matbandcigar=W@D <matrix_file> [gap_open gap_extend]:\n"
                "the lines of +band=W@D and of +bandcigar=W@D under the substitution matrix; a matrix file is required, and no\n"
                "+stats, +cigar or +zdrop.\n"
                "       %s <file_path> <mode>+dualband=W@D <match> <mismatch> <gap_open> <gap_extend> <gap_open2> <gap_extend2>\n"
                "the lines of +band=W@D under two-piece gap costs: a gap of L scores max(gap_open + L gap_extend, gap_open2 + L gap_extend2);\n"
                "all six integers are required, and no +stats, +cigar or +zdrop.\n"
                "       %s <file_path> <mode>+dualbandcigar=W@D <match> <mismatch> <gap_open> <gap_extend> <gap_open2> <gap_extend2>\n"
                "the same with its CIGAR inside that band appended, as +bandcigar=W@D formats it.\n",
                argv[0], argv[0], argv[0], argv[0]);
        return 1;
    }
    static agx_sw_matrix matrix;
    const int with_matrix = argc >= 4 && !with_dual;
    if (with_matrix) {
        char err[512];
        if (read_matrix(argv[3], &matrix, err, sizeof err)) {
            fprintf(stderr, "swAlign: %s\n", err);
            return EXIT_FAILURE;
        }
        matrix.gap_open = -11;
        matrix.gap_extend = -1;
        if (argc == 6) {
            char *e1, *e2;
            matrix.gap_open = (int32_t)strtol(argv[4], &e1, 10);
            matrix.gap_extend = (int32_t)strtol(argv[5], &e2, 10);
            if (e1 == argv[4] || *e1 || e2 == argv[5] || *e2) {
                fprintf(stderr, "swAlign: gap_open and gap_extend must be integers (got '%s' '%s')\n", argv[4], argv[5]);
                return EXIT_FAILURE;
            }
        }
    }
    const char *cp = getenv("AGX_CLI_CHUNK_PAIRS");
    const int64_t chunk_pairs = cp && atoll(cp) > 0 ? atoll(cp) : 262144;
    agx_sw_reader *reader = NULL;
    if (agx_sw_reader_open(argv[1], with_band ? 65536 : 0, &reader) != AGX_OK) {
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
            agx_sw_stat *stats = with_stats ? (agx_sw_stat *)malloc(sizeof(agx_sw_stat) * (size_t)t->n_pairs) : NULL;
            uint64_t *op_off = with_cigar ? (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)t->n_pairs + 1)) : NULL;
            uint32_t *ops = NULL;
            uint64_t ops_cap = 0; /* an alignment has at most one operation per symbol */
            for (int64_t k = 0; with_cigar && k < 2 * t->n_pairs; k++) ops_cap += t->len[k];
            if (with_cigar) ops = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(ops_cap + 1));
            if (!hits || (with_stats && !stats) || (with_cigar && (!op_off || !ops))) {
                fprintf(stderr, "swAlign: out of memory\n");
                status = EXIT_FAILURE;
            }
            if (!status && !ctx && agx_ctx_create(0, &ctx) != AGX_OK) {
                fprintf(stderr, "swAlign: %s\n", agx_last_error());
                status = EXIT_FAILURE;
            }
            if (with_matrix) /* a line's end is not a residue */
                for (int64_t k = 0; k < 2 * t->n_pairs; k++) {
                    if (t->len[k] && t->bases[t->off[k] + t->len[k] - 1] == '\n') t->len[k]--;
                    if (t->len[k] && t->bases[t->off[k] + t->len[k] - 1] == '\r') t->len[k]--;
                }
            if (!status && with_stats && with_diag) {
                int32_t *dg = (int32_t *)malloc(sizeof(int32_t) * (size_t)t->n_pairs);
                for (int64_t p = 0; dg && p < t->n_pairs; p++) dg[p] = diag;
                if (!dg) {
                    fprintf(stderr, "swAlign: out of memory\n");
                    status = EXIT_FAILURE;
                } else if (agx_sw_align_band_diag_stats(ctx, NULL, mode, band, dg, t->bases, t->off, t->len, t->n_pairs, hits, stats) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
                free(dg);
            } else if (!status && with_stats) {
                if (agx_sw_align_stats(ctx, NULL, with_matrix ? &matrix : NULL, mode, t->bases, t->off, t->len, t->n_pairs, hits, stats) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
            } else if (!status && with_cigar && with_diag) {
                int32_t *dg = (int32_t *)malloc(sizeof(int32_t) * (size_t)t->n_pairs);
                for (int64_t p = 0; dg && p < t->n_pairs; p++) dg[p] = diag;
                if (!dg) {
                    fprintf(stderr, "swAlign: out of memory\n");
                    status = EXIT_FAILURE;
                } else if ((with_dual ? agx_sw_align_band_diag_dual_cigar(ctx, &dual, mode, band, dg, t->bases, t->off, t->len, t->n_pairs, hits, op_off, ops,
                                                                          ops_cap)
                            : with_matband ? agx_sw_align_band_diag_matrix_cigar(ctx, &matrix, mode, band, dg, t->bases, t->off, t->len, t->n_pairs, hits,
                                                                               op_off, ops, ops_cap)
                            : with_zdrop ? agx_sw_align_band_zdrop_cigar(ctx, NULL, mode, band, dg, zdrop, t->bases, t->off, t->len, t->n_pairs, hits, NULL,
                                                                         op_off, ops, ops_cap)
                                         : agx_sw_align_band_diag_cigar(ctx, NULL, mode, band, dg, t->bases, t->off, t->len, t->n_pairs, hits, op_off, ops,
                                                                      ops_cap)) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
                free(dg);
            } else if (!status && with_cigar && with_band) {
                if (agx_sw_align_band_cigar(ctx, NULL, mode, band, t->bases, t->off, t->len, t->n_pairs, hits, op_off, ops, ops_cap) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
            } else if (!status && with_cigar) {
                if (agx_sw_align_cigar(ctx, NULL, with_matrix ? &matrix : NULL, mode, t->bases, t->off, t->len, t->n_pairs, hits, op_off, ops, ops_cap) !=
                    AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
            } else if (!status && with_diag) {
                int32_t *dg = (int32_t *)malloc(sizeof(int32_t) * (size_t)t->n_pairs);
                for (int64_t p = 0; dg && p < t->n_pairs; p++) dg[p] = diag;
                if (!dg) {
                    fprintf(stderr, "swAlign: out of memory\n");
                    status = EXIT_FAILURE;
                } else if ((with_dual ? agx_sw_align_band_diag_dual(ctx, &dual, mode, AGX_SW_ALIGN_SPANS, band, dg, t->bases, t->off, t->len, t->n_pairs,
                                                                    hits)
                            : with_matband ? agx_sw_align_band_diag_matrix(ctx, &matrix, mode, AGX_SW_ALIGN_SPANS, band, dg, t->bases, t->off, t->len,
                                                                         t->n_pairs, hits)
                            : with_zdrop ? agx_sw_align_band_zdrop(ctx, NULL, mode, AGX_SW_ALIGN_SPANS, band, dg, zdrop, t->bases, t->off, t->len,
                                                                   t->n_pairs, hits, NULL)
                                         : agx_sw_align_band_diag(ctx, NULL, mode, AGX_SW_ALIGN_SPANS, band, dg, t->bases, t->off, t->len, t->n_pairs,
                                                                hits)) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
                free(dg);
            } else if (!status && with_band) {
                if (agx_sw_align_band(ctx, NULL, mode, band, t->bases, t->off, t->len, t->n_pairs, hits) != AGX_OK) {
                    fprintf(stderr, "swAlign: %s\n", agx_last_error());
                    status = EXIT_FAILURE;
                }
            } else if (!status && (with_matrix ? agx_sw_align_matrix(ctx, &matrix, mode, AGX_SW_ALIGN_SPANS, t->bases, t->off, t->len, t->n_pairs, hits)
                                        : agx_sw_align_mode(ctx, NULL, mode, AGX_SW_ALIGN_SPANS, t->bases, t->off, t->len, t->n_pairs, hits)) != AGX_OK) {
                fprintf(stderr, "swAlign: %s\n", agx_last_error());
                status = EXIT_FAILURE;
            }
            if (!status && with_stats)
                for (int64_t p = 0; p < t->n_pairs; p++)
                    printf("%d %d %d %d %d %d %d\n", hits[p].score, hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end, stats[p].matches,
                           stats[p].pairs);
            else if (!status && with_cigar)
                for (int64_t p = 0; p < t->n_pairs; p++) {
                    printf("%d %d %d %d %d ", hits[p].score, hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end);
                    for (uint64_t k = op_off[p]; k < op_off[p + 1]; k++) {
                        const unsigned op = ops[k] & 15u;
                        printf("%u%c", ops[k] >> 4, op == AGX_CIGAR_INS ? 'I' : op == AGX_CIGAR_DEL ? 'D' : op == AGX_CIGAR_EQ ? '=' : 'X');
                    }
                    printf(op_off[p] == op_off[p + 1] ? "*\n" : "\n");
                }
            else if (!status)
                for (int64_t p = 0; p < t->n_pairs; p++)
                    printf("%d %d %d %d %d\n", hits[p].score, hits[p].a_begin, hits[p].a_end, hits[p].b_begin, hits[p].b_end);
            free(hits);
            free(stats);
            free(op_off);
            free(ops);
        }
        agx_sw_text_free(t);
    }
    agx_sw_reader_close(reader);
    if (ctx) agx_ctx_destroy(ctx);
    return status;
}
