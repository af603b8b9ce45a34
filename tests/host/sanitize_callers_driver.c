/*
 * Host-only driver with several CALLERS for the ThreadSanitizer build (tests/test_callers_sanitizers.py): four pthreads enter
 * the library at once, where tests/host/sanitize_driver.c has one caller and the pool's threads.  Every caller makes plan-only
 * creates (ctx == NULL: no device is touched) of every batch family from inputs all callers share and only read; two of them
 * also run the text readers, on golden files and on two files the driver writes itself, large enough for the readers' own
 * pool to split them.  Every result is compared with the one made before the callers started.
 * usage: sanitize_callers_driver <golden dir> <scratch dir>
 */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "agx.h"

#define CALLERS 4
#define ROUNDS 2

static int fails = 0; /* written by the main thread, and by callers under fail_mu */
static pthread_mutex_t fail_mu = PTHREAD_MUTEX_INITIALIZER;
#define EXPECT(c)                                                               \
    do {                                                                        \
        if (!(c)) {                                                             \
            pthread_mutex_lock(&fail_mu);                                       \
            fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #c, agx_last_error()); \
            fails++;                                                            \
            pthread_mutex_unlock(&fail_mu);                                     \
        }                                                                       \
    } while (0)

static uint32_t lcg(uint32_t *s) { return *s = *s * 1664525u + 1013904223u; }

/* ------------------------------------------------------------------ shared inputs */

typedef struct sw_input {
    uint8_t *bases;
    uint64_t *off;
    uint32_t *len;
    int32_t *diag;
    int64_t n;
} sw_input;

static sw_input sw_make(int64_t n, uint32_t lo, uint32_t hi, const char *alphabet, uint32_t seed)
{
    sw_input b;
    const uint32_t na = (uint32_t)strlen(alphabet);
    b.n = n;
    b.off = malloc(2 * (size_t)n * sizeof *b.off);
    b.len = malloc(2 * (size_t)n * sizeof *b.len);
    b.diag = malloc((size_t)n * sizeof *b.diag);
    uint64_t total = 0;
    for (int64_t k = 0; k < 2 * n; k++) {
        b.len[k] = lo + lcg(&seed) % (hi - lo + 1);
        b.off[k] = total;
        total += b.len[k];
    }
    b.bases = malloc(total + 1);
    for (uint64_t k = 0; k < total; k++) b.bases[k] = (uint8_t)alphabet[(lcg(&seed) >> 8) % na];
    for (int64_t p = 0; p < n; p++) b.diag[p] = (int32_t)(lcg(&seed) >> 8) % 9 - 4;
    return b;
}

static void sw_free(sw_input *b) { free(b->bases), free(b->off), free(b->len), free(b->diag); }

typedef struct phmm_input {
    agx_phmm_desc d;
    void *own[7];
} phmm_input;

static phmm_input phmm_make(uint32_t n_regions, uint32_t reads_per, uint32_t haps_per, uint32_t r_lo, uint32_t r_hi, uint32_t h_lo, uint32_t h_hi)
{
    uint32_t seed = 4242u;
    const uint32_t nr = n_regions * reads_per, nh = n_regions * haps_per;
    uint64_t *roff = calloc(nr + 1, sizeof *roff), *hoff = calloc(nh + 1, sizeof *hoff);
    uint32_t *rreg = calloc(n_regions + 1, sizeof *rreg), *hreg = calloc(n_regions + 1, sizeof *hreg);
    for (uint32_t r = 0; r < nr; r++) roff[r + 1] = roff[r] + r_lo + lcg(&seed) % (r_hi - r_lo + 1);
    for (uint32_t h = 0; h < nh; h++) hoff[h + 1] = hoff[h] + h_lo + lcg(&seed) % (h_hi - h_lo + 1);
    for (uint32_t g = 0; g <= n_regions; g++) rreg[g] = g * reads_per, hreg[g] = g * haps_per;
    uint8_t *rb = malloc(roff[nr] + 1), *q = malloc(roff[nr] + 1), *hb = malloc(hoff[nh] + 1);
    for (uint64_t k = 0; k < roff[nr]; k++) {
        rb[k] = (uint8_t)"ACGT"[(lcg(&seed) >> 8) % 4u];
        q[k] = (uint8_t)(33 + 10 + (lcg(&seed) >> 8) % 30u);
    }
    for (uint64_t k = 0; k < hoff[nh]; k++) hb[k] = (uint8_t)"ACGT"[(lcg(&seed) >> 8) % 4u];
    phmm_input p;
    memset(&p, 0, sizeof p);
    p.d.read_bases = rb, p.d.q_base = q, p.d.q_ins = q, p.d.q_del = q, p.d.q_gcp = q;
    p.d.read_off = roff, p.d.n_reads = nr;
    p.d.hap_bases = hb, p.d.hap_off = hoff, p.d.n_haps = nh;
    p.d.region_read = rreg, p.d.region_hap = hreg, p.d.n_regions = n_regions;
    void *own[7] = {roff, hoff, rreg, hreg, rb, q, hb};
    memcpy(p.own, own, sizeof own);
    return p;
}

static void phmm_free(phmm_input *p)
{
    for (int k = 0; k < 7; k++) free(p->own[k]);
}

static sw_input dna, near, protein;
static phmm_input phmm;
static agx_sw_matrix m20, m4;
static const agx_sw_scoring scored = {2, -3, -5, -2}, dna_scoring = {2, -4, -4, -2};

static void matrix_make(agx_sw_matrix *m, const char *alphabet, int gap_open, int gap_extend)
{
    const int n = (int)strlen(alphabet);
    memset(m, 0, sizeof *m);
    m->n_symbols = n;
    m->gap_open = gap_open;
    m->gap_extend = gap_extend;
    memset(m->code, 0xff, sizeof m->code);
    for (int k = 0; k < n; k++) m->code[(unsigned char)alphabet[k]] = (uint8_t)k;
    for (int a = 0; a < n; a++)
        for (int c = 0; c < n; c++) m->score[a][c] = (int8_t)(a == c ? 5 : (a + c) % 5 - 3); /* symmetric; 0 and positive off the diagonal */
}

/* ------------------------------------------------------------------ the plan-only creates */

typedef struct result {
    int rc;
    int64_t v[8]; /* every field of the batch's info */
} result;

static result of_sw(int rc, agx_sw_batch *b)
{
    result r;
    memset(&r, 0, sizeof r);
    r.rc = rc;
    agx_sw_info i;
    if (!rc && b && agx_sw_batch_info(b, &i) == AGX_OK) {
        const int64_t v[8] = {i.n_pairs, i.cells, i.padded_cells, i.input_bytes, i.n_launches, i.n_waves, i.planned_on_device, 1};
        memcpy(r.v, v, sizeof v);
    }
    agx_sw_batch_destroy(b);
    return r;
}

static result of_phmm(int precision)
{
    result r;
    memset(&r, 0, sizeof r);
    agx_phmm_batch *b = NULL;
    r.rc = agx_phmm_batch_create(NULL, &phmm.d, precision, &b);
    agx_phmm_info i;
    if (!r.rc && b && agx_phmm_batch_info(b, &i) == AGX_OK) {
        const int64_t v[8] = {i.n_pairs, i.cells, i.padded_cells, i.input_bytes, i.n_launches, i.n_waves, i.n_rescued, 1};
        memcpy(r.v, v, sizeof v);
    }
    agx_phmm_batch_destroy(b);
    return r;
}

#define SW(in) (in).bases, (in).off, (in).len, (in).n, &b
enum { L = AGX_SW_MODE_LOCAL, G = AGX_SW_MODE_GLOBAL, F = AGX_SW_MODE_FIT, E = AGX_SW_MODE_EXTEND, ENDS = AGX_SW_ALIGN_ENDS, SPANS = AGX_SW_ALIGN_SPANS };
#define N_CASES 24

static result create(int k)
{
    agx_sw_batch *b = NULL;
    switch (k) {
    case 0: return of_sw(agx_sw_batch_create(NULL, SW(dna)), b);
    case 1: return of_sw(agx_sw_batch_create_scored(NULL, &scored, SW(dna)), b);
    case 2: return of_sw(agx_sw_batch_create_matrix(NULL, &m20, SW(protein)), b);
    case 3: return of_sw(agx_sw_batch_create_align(NULL, NULL, ENDS, SW(dna)), b);
    case 4: return of_sw(agx_sw_batch_create_align(NULL, NULL, SPANS, SW(dna)), b);
    case 5: return of_sw(agx_sw_batch_create_align_mode(NULL, NULL, F, ENDS, SW(dna)), b);
    case 6: return of_sw(agx_sw_batch_create_align_mode(NULL, &scored, G, SPANS, SW(dna)), b);
    case 7: return of_sw(agx_sw_batch_create_align_matrix(NULL, &m20, F, SPANS, SW(protein)), b);
    case 8: return of_sw(agx_sw_batch_create_align_stats(NULL, NULL, NULL, L, SW(dna)), b);
    case 9: return of_sw(agx_sw_batch_create_align_stats(NULL, NULL, NULL, G, SW(dna)), b);
    case 10: return of_sw(agx_sw_batch_create_align_cigar(NULL, NULL, NULL, F, SW(dna)), b);
    case 11: return of_sw(agx_sw_batch_create_align_band(NULL, NULL, G, 32, SW(near)), b);
    case 12: return of_sw(agx_sw_batch_create_align_band_cigar(NULL, NULL, E, 32, SW(near)), b);
    case 13: return of_sw(agx_sw_batch_create_align_band_diag(NULL, NULL, L, SPANS, 16, near.diag, SW(near)), b);
    case 14: return of_sw(agx_sw_batch_create_align_band_diag(NULL, NULL, F, ENDS, 40, near.diag, SW(near)), b);
    case 15: return of_sw(agx_sw_batch_create_align_band_diag_matrix(NULL, &m4, L, SPANS, 16, near.diag, SW(near)), b);
    case 16: return of_sw(agx_sw_batch_create_align_band_diag_cigar(NULL, NULL, L, 16, near.diag, SW(near)), b);
    case 17: return of_sw(agx_sw_batch_create_align_band_zdrop(NULL, &dna_scoring, E, SPANS, 16, near.diag, 20, SW(near)), b);
    case 18: return of_phmm(AGX_PHMM_F64);
    case 19: return of_phmm(AGX_PHMM_F64_FMA);
    case 20: return of_phmm(AGX_PHMM_F32);
    case 21: return of_phmm(AGX_PHMM_F32_FMA);
    case 22: return of_phmm(AGX_PHMM_F64 | AGX_PHMM_GATK_PRIOR);
    default: return of_phmm(AGX_PHMM_F32_FMA | AGX_PHMM_GATK_PRIOR);
    }
}

/* ------------------------------------------------------------------ the text readers */

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = p;
    for (size_t k = 0; k < n; k++) h = (h ^ b[k]) * 1099511628211ull;
    return h;
}

static uint64_t sw_text_hash(uint64_t h, const agx_sw_text *t)
{
    const size_t n = 2 * (size_t)t->n_pairs;
    h = fnv(h, &t->line_num, sizeof t->line_num);
    h = fnv(h, &t->n_pairs, sizeof t->n_pairs);
    h = fnv(h, t->off, n * sizeof *t->off);
    h = fnv(h, t->len, n * sizeof *t->len);
    for (size_t k = 0; k < n; k++) h = fnv(h, t->bases + t->off[k], t->len[k]);
    if (t->dangling) h = fnv(h, t->dangling, strlen(t->dangling));
    return h;
}

static uint64_t phmm_text_hash(const agx_phmm_text *t)
{
    const agx_phmm_desc *d = &t->desc;
    uint64_t h = fnv(14695981039346656037ull, &t->n_pairs, sizeof t->n_pairs);
    h = fnv(h, d->read_off, ((size_t)d->n_reads + 1) * sizeof *d->read_off);
    h = fnv(h, d->hap_off, ((size_t)d->n_haps + 1) * sizeof *d->hap_off);
    h = fnv(h, d->region_read, ((size_t)d->n_regions + 1) * sizeof *d->region_read);
    h = fnv(h, d->region_hap, ((size_t)d->n_regions + 1) * sizeof *d->region_hap);
    const size_t nb = d->n_reads ? (size_t)d->read_off[d->n_reads] : 0;
    h = fnv(h, d->read_bases, nb), h = fnv(h, d->q_base, nb), h = fnv(h, d->q_ins, nb), h = fnv(h, d->q_del, nb), h = fnv(h, d->q_gcp, nb);
    return fnv(h, d->hap_bases, d->n_haps ? (size_t)d->hap_off[d->n_haps] : 0);
}

static char sw_path[2][1024], phmm_path[2][1024];

/* what[0..1]: the SW files whole, [2..3]: the same through the chunked reader (chunks hashed one after the other), [4..5]: PairHMM */
static void read_all(uint64_t what[6])
{
    for (int f = 0; f < 2; f++) {
        agx_sw_text *t = NULL;
        EXPECT(agx_sw_text_read(sw_path[f], 0, &t) == AGX_OK && t);
        what[f] = t ? sw_text_hash(14695981039346656037ull, t) : 0;
        agx_sw_text_free(t);
        agx_sw_reader *r = NULL;
        EXPECT(agx_sw_reader_open(sw_path[f], 0, &r) == AGX_OK && r);
        uint64_t h = 14695981039346656037ull;
        while (r && !agx_sw_reader_done(r)) {
            agx_sw_text *c = NULL;
            EXPECT(agx_sw_reader_next(r, 40000, &c) == AGX_OK && c);
            if (!c) break;
            h = sw_text_hash(h, c);
            agx_sw_text_free(c);
        }
        agx_sw_reader_close(r);
        what[2 + f] = h;
        agx_phmm_text *p = NULL;
        EXPECT(agx_phmm_text_read(phmm_path[f], &p) == AGX_OK && p);
        what[4 + f] = p ? phmm_text_hash(p) : 0;
        agx_phmm_text_free(p);
    }
}

/* 66 000 lines of 100..199 symbols: about 10 MB, which the reader splits into parts of 4 MB on its pool */
static void write_sw_file(const char *path)
{
    FILE *f = fopen(path, "w");
    if (!f) {
        fails++;
        return;
    }
    uint32_t seed = 77u;
    char line[256];
    fprintf(f, "%d\n", 66000);
    for (int k = 0; k < 66000; k++) {
        const int n = 100 + (int)(lcg(&seed) % 100u);
        for (int i = 0; i < n; i++) line[i] = "ACGT"[(lcg(&seed) >> 8) % 4u];
        line[n] = '\n';
        fwrite(line, 1, (size_t)n + 1, f);
    }
    fclose(f);
}

/* 6 regions of 400 reads x 3 haplotypes: the read lines of a region are cut into their fields on the readers' pool from 256 reads on */
static void write_phmm_file(const char *path)
{
    FILE *f = fopen(path, "w");
    if (!f) {
        fails++;
        return;
    }
    uint32_t seed = 78u;
    char s[5][128];
    for (int g = 0; g < 6; g++) {
        fprintf(f, "%d %d\n", 400, 3);
        for (int r = 0; r < 400; r++) {
            const int n = 40 + (int)(lcg(&seed) % 60u);
            for (int i = 0; i < n; i++) {
                s[0][i] = "ACGT"[(lcg(&seed) >> 8) % 4u];
                for (int k = 1; k < 5; k++) s[k][i] = (char)(33 + 10 + (lcg(&seed) >> 8) % 30u);
            }
            for (int k = 0; k < 5; k++) s[k][n] = 0;
            fprintf(f, "%s %s %s %s %s\n", s[0], s[1], s[2], s[3], s[4]);
        }
        for (int h = 0; h < 3; h++) {
            const int n = 110 + (int)(lcg(&seed) % 10u);
            for (int i = 0; i < n; i++) s[0][i] = "ACGT"[(lcg(&seed) >> 8) % 4u];
            s[0][n] = 0;
            fprintf(f, "%s\n", s[0]);
        }
    }
    fclose(f);
}

/* ------------------------------------------------------------------ the callers */

static result alone[N_CASES];
static uint64_t read_alone[6];
static pthread_barrier_t gate;

static void *caller(void *arg)
{
    const int t = (int)(intptr_t)arg;
    pthread_barrier_wait(&gate);
    for (int round = 0; round < ROUNDS; round++) {
        for (int i = 0; i < N_CASES; i++) {
            const int k = (i + t * N_CASES / CALLERS) % N_CASES; /* every caller in another rotation */
            const result r = create(k);
            if (r.rc != alone[k].rc || memcmp(r.v, alone[k].v, sizeof r.v)) {
                pthread_mutex_lock(&fail_mu);
                fprintf(stderr, "FAIL caller %d round %d case %d: rc %d (alone %d), info", t, round, k, r.rc, alone[k].rc);
                for (int j = 0; j < 8; j++) fprintf(stderr, " %lld/%lld", (long long)r.v[j], (long long)alone[k].v[j]);
                fprintf(stderr, "\n");
                fails++;
                pthread_mutex_unlock(&fail_mu);
            }
            if (t < 2 && i % (N_CASES / 2) == 3 * t) { /* twice a round, at different places in the two callers' lists */
                uint64_t got[6];
                read_all(got);
                EXPECT(memcmp(got, read_alone, sizeof got) == 0);
            }
        }
    }
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    snprintf(sw_path[0], sizeof sw_path[0], "%s/sw_mixed.in", argv[1]);
    snprintf(phmm_path[0], sizeof phmm_path[0], "%s/phmm_10s.in", argv[1]);
    snprintf(sw_path[1], sizeof sw_path[1], "%s/callers_sw.in", argv[2]);
    snprintf(phmm_path[1], sizeof phmm_path[1], "%s/callers_phmm.in", argv[2]);
    write_sw_file(sw_path[1]);
    write_phmm_file(phmm_path[1]);
    dna = sw_make(70000, 32, 128, "ACGT", 1u);     /* 8 parts of 8192 pairs; counting sorts of 2 parts of 32 768 */
    near = sw_make(20000, 100, 130, "ACGT", 2u);   /* |la - lb| <= 30: a band of 32 holds the end corner */
    protein = sw_make(20000, 20, 120, "ARNDCQEGHILKMFPSTWYV", 3u);
    phmm = phmm_make(48, 64, 16, 40, 100, 240, 300); /* 49 152 pairs: 3 parts of 16 384 */
    matrix_make(&m20, "ARNDCQEGHILKMFPSTWYV", -11, -1);
    matrix_make(&m4, "ACGT", -2, -1);

    for (int k = 0; k < N_CASES; k++) {
        alone[k] = create(k);
        EXPECT(alone[k].rc == AGX_OK && alone[k].v[7] == 1 && alone[k].v[0] >= 16384 && alone[k].v[5] > 0);
    }
    read_all(read_alone);
    for (int k = 0; k < 6; k++) EXPECT(read_alone[k] != 0);

    pthread_t th[CALLERS];
    pthread_barrier_init(&gate, NULL, CALLERS);
    for (int t = 0; t < CALLERS; t++)
        if (pthread_create(&th[t], NULL, caller, (void *)(intptr_t)t)) return 3;
    for (int t = 0; t < CALLERS; t++) pthread_join(th[t], NULL);
    pthread_barrier_destroy(&gate);

    sw_free(&dna), sw_free(&near), sw_free(&protein), phmm_free(&phmm);
    remove(sw_path[1]);
    remove(phmm_path[1]);
    printf(fails ? "SANITIZE_CALLERS_FAILED %d\n" : "SANITIZE_CALLERS_OK\n", fails);
    return fails ? 1 : 0;
}
