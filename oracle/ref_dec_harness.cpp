// ref_dec_harness.cpp -- TEST INFRASTRUCTURE ONLY.
//
// A thin extern "C" wrapper (our own code) around the REFERENCE's unmodified
// decoder source dec.cpp, compiled in place by oracle/Makefile together with
// the loader sources of libref.so into oracle/_ref/librefdec.so.  The decode
// loops are the reference's own Run_* functions; nothing of them is restated
// here.  Two stand-ins make dec.cpp build outside MSVC + MKL, and neither
// touches the decoders' arithmetic:
//   - oracle/stub/mkl_vsl.h, an empty header (rand.h:8 includes MKL's; dec.cpp
//     uses rand.h for the prototype of rand_int only);
//   - -D_isnan(x)=std::isnan(x): MSVC's _isnan and std::isnan are the same
//     predicate on a double.
// rand_int (rand.cpp:84, MKL's stream) is called solely to break the ties of
// the quantised min-sum (dec.cpp:1273, :1647).  It is defined here: it counts
// its calls and returns 0, or serves a caller's queue of bits.
//
// The reference keeps one matrix per process (rcode.cpp:33 H), so a load
// replaces the previous one.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mod2sparse.h"
#include "rcode.h"
#include "check.h"
#include "dec.h"
#include "common.h"

static int64_t g_ties, g_queue_len, g_queue_pos, g_underrun;
static const uint8_t *g_queue;

// dec.cpp:1273, :1647 call rand_int(2) once per zero prior / zero posterior.
int rand_int(int r)
{
    (void)r;
    g_ties++;
    if (!g_queue) return 0;
    if (g_queue_pos >= g_queue_len) { g_underrun++; return 0; }
    return g_queue[g_queue_pos++] != 0;
}

extern "C" {

// read_pchk() exits the process on error: callers pass a known-good file.
// CheckRegular sets the globals D_v / D_c that Gallager's thresholds read
// (dec.cpp:777-779, :811-813).
int refdec_load(const char *path, int *M_out, int *N_out, int *dv_out, int *dc_out)
{
    if (H) { mod2sparse_free(H); H = NULL; }
    read_pchk((char *)path);
    CheckRegular(H);
    *M_out = mod2sparse_rows(H);
    *N_out = mod2sparse_cols(H);
    *dv_out = D_v;
    *dc_out = D_c;
    return 0;
}

int64_t refdec_ties(void) { return g_ties; }

// Serve the next rand_int calls from bits[0..n) (NULL: return 0 again).
void refdec_tie_queue(const uint8_t *bits, int64_t n)
{
    g_queue = bits; g_queue_len = n; g_queue_pos = 0; g_underrun = 0;
}

// Bits of the queue left unread (> 0: overrun of the caller's guess) and
// calls that found it empty.
void refdec_tie_queue_state(int64_t *unread, int64_t *underrun)
{
    *unread = g_queue ? g_queue_len - g_queue_pos : 0;
    *underrun = g_underrun;
}

// Run_Belief_Propagation_Decoder on lratio as given (the LR domain).  post
// receives lratio[j] times the column's e->lr in list order with NaN -> 1:
// our walk over the reference's own entries, the product that dec.cpp:669-677
// forms before it decides.
int refdec_bp(const double *lratio, int iters, uint8_t *dblk, double *post, int *valid)
{
    int ok = 0, n;
    char *pchk = (char *)calloc((size_t)mod2sparse_rows(H) + 1, 1);
    max_iter = iters;
    n = Run_Belief_Propagation_Decoder(H, (double *)lratio, (char *)dblk, pchk, &ok);
    if (post) {
        for (int j = 0; j < mod2sparse_cols(H); j++) {
            double p = lratio[j];
            for (mod2entry *e = mod2sparse_first_in_col(H, j); !mod2sparse_at_end(e); e = mod2sparse_next_in_col(e))
                p *= e->lr;
            post[j] = std::isnan(p) ? 1 : p;
        }
    }
    *valid = ok;
    free(pchk);
    return n;
}

// Run_MSA_Decoder_INF.  It leaves L unwritten when it stops at n = 0; L is
// preset to the LLR there, as the oracle and the product define it.
int refdec_msa(const double *llr, int iters, uint8_t *dblk, double *L, int *valid)
{
    int ok = 0, n;
    char *pchk = (char *)calloc((size_t)mod2sparse_rows(H) + 1, 1);
    max_iter = iters;
    memcpy(L, llr, sizeof(double) * (size_t)mod2sparse_cols(H));
    n = Run_MSA_Decoder_INF(H, (double *)llr, L, (char *)dblk, pchk, &ok);
    *valid = ok;
    free(pchk);
    return n;
}

// Run_Gallager_Decoder, type 0 / 1 / 2 = A / B1 / B2, on recv in {-1, +1}.
int refdec_gallager(const int *recv, int type, int iters, uint8_t *dblk, int *valid)
{
    int ok = 0, n;
    char *pchk = (char *)calloc((size_t)mod2sparse_rows(H) + 1, 1);
    max_iter = iters;
    n = Run_Gallager_Decoder(H, (int *)recv, (char *)dblk, pchk, type, &ok);
    *valid = ok;
    free(pchk);
    return n;
}

// Set_MSA + Cal_MSA_Q(x, 0) on n values.
void refdec_quantise(const double *x, int64_t n, int q, double step, int beta, int *out)
{
    Set_MSA(q, step, beta);
    for (int64_t i = 0; i < n; i++) out[i] = Cal_MSA_Q(x[i], 0);
}

// Set_MSA, Cal_MSA_Q per position, Run_MSA_Decoder with no state files
// (bSave_word_state stays 0).  L_Q is preset to the quantised prior for a stop
// at n = 0.  *ties receives the number of rand_int calls of this decode.
int refdec_qmsa(const double *llr, int q, double step, int beta, int iters, uint8_t *dblk, int *L_Q, int *valid,
                int64_t *ties)
{
    int ok = 0, n, N = mod2sparse_cols(H);
    char *pchk = (char *)calloc((size_t)mod2sparse_rows(H) + 1, 1);
    int *qllr = (int *)malloc(sizeof(int) * (size_t)N);
    int64_t t0 = g_ties;
    Set_MSA(q, step, beta);
    for (int j = 0; j < N; j++) L_Q[j] = qllr[j] = Cal_MSA_Q(llr[j], 0);
    bSave_word_state = 0;
    max_iter = iters;
    n = Run_MSA_Decoder(H, qllr, L_Q, (char *)dblk, pchk, &ok, NULL, NULL, NULL);
    *valid = ok;
    *ties = g_ties - t0;
    free(qllr);
    free(pchk);
    return n;
}

}  // extern "C"
