/* Exhaustive proof for the device's quadrant word and fused Cody-Waite step in Julia's Float32 sin / cos
 * (include/srhip_math.h srm_jqword / srm_jqword_wide / srm_jred_cw_fma, srhip_eval_impl.h jtrigf_*),
 * over all 2^32 inputs, per tier and kind (0: cos, 1: sin).  Exit status 1 on any difference.
 *
 *  (1) srm_jred_cw_fma returns srm_jred_cw's double, bit for bit, on every float below 2^28 pi/2.
 *  (2) srm_jqword's bits 30 and 31 equal n1 & 1 and (n1 >> 1) & 1 (n1 = (int)fn + 1 - kind) on every
 *      |x| < SRM_JQW_MAXF -- every input tiers B and C may see; srm_jqword_wide's bits 21 and 22 equal them
 *      on every float below 2^28 pi/2 -- every row the slow body's fast path may see.
 *  (3) SRM_JQW_MAXF is the largest bound of tier C's wave test (mx < bound) that keeps |fn| < 2^20:
 *      every |x| below it gives |fn| < 2^20, and x = SRM_JQW_MAXF itself gives fn = 2^20.
 *  (4) the composed new row (reduction, quadrant word, Horner kernels, select, sign from the word) returns
 *      srm_jtrigf's bits on every input its tie test leaves unflagged, for tier B, tier C and the slow
 *      body's fast rows, and flags exactly the inputs the integer-quadrant row (tools/check_trigf.c
 *      tier_bc_fast) flags.  (sin keeps x where x == 0: per row in the slow body and in a wave of tier
 *      B / C that holds a zero; a wave without one skips a select that would have kept every r.)
 *  SRHIP_TIE_DUMP=<file>: also write every flagged input (uint32 bits, any tier / kind, tier A included,
 *  ascending) -- it must reproduce tests/golden/trig_tie_inputs.npy's payload.
 * Build: gcc -O2 -march=x86-64-v3 -ffp-contract=off -fopenmp tools/check_trig_quadrant.c -lm -o check_trig_quadrant */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/srhip_math.h"

#define BIG_F 421657440.0f /* Float32(2^28 pi/2): at and above it a row takes the scalar srm_jtrigf */

static float from_u(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t to_u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t to_u64(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

/* tier A's fast row, as tools/check_trigf.c states it (unchanged: for the flagged-input dump only) */
static int tier_a_flag(int kind, float x) {
  const double xd = (double)x, z = xd * xd;
  return srm_jtie(kind == 0 ? srm_jcos_fma(z) : srm_jsin_fma(xd, z));
}
/* the integer-quadrant row this change replaces (tools/check_trigf.c tier_bc_fast) */
static float row_old(int kind, float x, int cw, int* flag) {
  const double xd = (double)x, fn = srm_jfn(xd);
  double y = srm_jred_near(xd, fn);
  if (cw) y = kind == 0 ? srm_jred_cw(xd, fn) : (fabsf(x) <= SRM_J9PIO4F ? y : srm_jred_cw(xd, fn));
  const int n = (int)fn;
  const double z = y * y;
  const double p = ((n & 1) ^ kind) ? srm_jsin_fma(y, z) : srm_jcos_fma(z);
  *flag = srm_jtie(p);
  const float r = (float)p;
  const float q = (((n + 1 - kind) >> 1) & 1) ? -r : r;
  return (kind == 1 && x == 0.0f) ? x : q;
}
/* the new row: cw 0 tier B, 1 tier C, 2 a fast row of the slow body (the wide word) */
static float row_new(int kind, float x, int cw, int* flag) {
  const double xd = (double)x, fn = srm_jfn(xd);
  double y = srm_jred_near(xd, fn);
  if (cw) y = kind == 0 ? srm_jred_cw_fma(xd, fn) : (fabsf(x) <= SRM_J9PIO4F ? y : srm_jred_cw_fma(xd, fn));
  const uint32_t w = cw == 2 ? srm_jqword_wide(kind, fn) << 9 : srm_jqword(kind, fn);
  const double z = y * y;
  const double p = (w & 0x40000000u) ? srm_jcos_fma(z) : srm_jsin_fma(y, z);
  *flag = srm_jtie(p);
  const float r = from_u(to_u((float)p) ^ (w & 0x80000000u));
  return (kind == 1 && x == 0.0f) ? x : r;
}

static int cmp_u32(const void* a, const void* b) {
  const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return (x > y) - (x < y);
}

int main(void) {
  const float bound = SRM_JQW_MAXF;
  /* (3), the upper half: the bound itself reaches fn = 2^20, so no larger bound of `mx < bound` is valid */
  const double fn_at = srm_jfn((double)bound), fn_below = srm_jfn((double)nextafterf(bound, 0.0f));
  printf("SRM_JQW_MAXF = %.9g (0x%08x): fn = %.1f there, %.1f at the float below\n", (double)bound, to_u(bound), fn_at,
         fn_below);
  if (!(fn_at == 1048576.0 && fn_below == 1048575.0 && bound < BIG_F)) {
    printf("SRM_JQW_MAXF is not the smallest float whose fn reaches 2^20\n");
    return 1;
  }
  const char* dump = getenv("SRHIP_TIE_DUMP");
  uint32_t* flagged = NULL;
  size_t nflagged = 0, cap = 1 << 16;
  if (dump && *dump) flagged = (uint32_t*)malloc(cap * sizeof(uint32_t));
  int status = 0;
  for (int kind = 0; kind < 2; ++kind) {
    uint64_t n_all = 0, n_bc = 0, n_b = 0, red = 0, wq = 0, wwide = 0, fnbig = 0;
    uint64_t bad_b = 0, bad_c = 0, bad_s = 0, fl_b = 0, fl_c = 0, fl_s = 0, fdiff = 0;
#pragma omp parallel for schedule(dynamic, 1 << 16) \
    reduction(+ : n_all, n_bc, n_b, red, wq, wwide, fnbig, bad_b, bad_c, bad_s, fl_b, fl_c, fl_s, fdiff)
    for (int64_t i = 0; i < (1LL << 32); ++i) {
      const float x = from_u((uint32_t)i);
      if (!(fabsf(x) < BIG_F)) continue; /* Inf / NaN / Payne-Hanek rows: the scalar srm_jtrigf itself */
      ++n_all;
      const double xd = (double)x, fn = srm_jfn(xd);
      const int n1 = (int)fn + 1 - kind;
      const uint32_t want = to_u(srm_jtrigf(kind, x));
      int any = 0, f_new, f_old;
      /* (1) the fused first step */
      red += to_u64(srm_jred_cw_fma(xd, fn)) != to_u64(srm_jred_cw(xd, fn));
      /* (2) the wide word */
      const uint32_t ww = srm_jqword_wide(kind, fn);
      wwide += ((ww >> 21) & 1u) != (uint32_t)(n1 & 1) || ((ww >> 22) & 1u) != (uint32_t)((n1 >> 1) & 1);
      /* (4) a fast row of the slow body */
      uint32_t got = to_u(row_new(kind, x, 2, &f_new));
      (void)row_old(kind, x, 1, &f_old);
      fl_s += f_new; fdiff += f_new != f_old; bad_s += !f_new && got != want;
      any |= f_new;
      if (fabsf(x) < bound) {
        ++n_bc;
        /* (3), the lower half */
        fnbig += !(fabs(fn) < 1048576.0);
        /* (2) the word of tiers B and C */
        const uint32_t w = srm_jqword(kind, fn);
        wq += ((w >> 30) & 1u) != (uint32_t)(n1 & 1) || (w >> 31) != (uint32_t)((n1 >> 1) & 1);
        /* (4) tier C */
        got = to_u(row_new(kind, x, 1, &f_new));
        (void)row_old(kind, x, 1, &f_old);
        fl_c += f_new; fdiff += f_new != f_old; bad_c += !f_new && got != want;
        any |= f_new;
      }
      if (fabsf(x) <= SRM_J9PIO4F) {
        ++n_b;
        /* (4) tier B */
        got = to_u(row_new(kind, x, 0, &f_new));
        (void)row_old(kind, x, 0, &f_old);
        fl_b += f_new; fdiff += f_new != f_old; bad_b += !f_new && got != want;
        any |= f_new;
      }
      if (flagged) {
        if (fabsf(x) < SRM_JPIO4F) any |= tier_a_flag(kind, x);
        if (any) {
#pragma omp critical
          {
            if (nflagged == cap) flagged = (uint32_t*)realloc(flagged, (cap *= 2) * sizeof(uint32_t));
            flagged[nflagged++] = (uint32_t)i;
          }
        }
      }
    }
    const char* k = kind ? "sin" : "cos";
    printf("%s reduction: %llu inputs, fused first step differs on %llu\n", k, (unsigned long long)n_all,
           (unsigned long long)red);
    printf("%s quadrant word: %llu inputs below the bound, %llu with |fn| >= 2^20, bits 30 / 31 differ on %llu; "
           "wide word: %llu inputs, bits 21 / 22 differ on %llu\n",
           k, (unsigned long long)n_bc, (unsigned long long)fnbig, (unsigned long long)wq, (unsigned long long)n_all,
           (unsigned long long)wwide);
    printf("%s new rows vs srm_jtrigf (flagged rows / unflagged wrong): B %llu inputs %llu / %llu, "
           "C %llu inputs %llu / %llu, slow %llu inputs %llu / %llu; flag differs from the integer-quadrant row on %llu\n",
           k, (unsigned long long)n_b, (unsigned long long)fl_b, (unsigned long long)bad_b, (unsigned long long)n_bc,
           (unsigned long long)fl_c, (unsigned long long)bad_c, (unsigned long long)n_all, (unsigned long long)fl_s,
           (unsigned long long)bad_s, (unsigned long long)fdiff);
    fflush(stdout);
    if (red || wq || wwide || fnbig || bad_b || bad_c || bad_s || fdiff) status = 1;
  }
  if (flagged) {
    /* both kinds' passes list an input flagged for either: sort and drop the repeats */
    qsort(flagged, nflagged, sizeof(uint32_t), cmp_u32);
    size_t m = 0;
    for (size_t j = 0; j < nflagged; ++j)
      if (m == 0 || flagged[m - 1] != flagged[j]) flagged[m++] = flagged[j];
    FILE* df = fopen(dump, "wb");
    if (!df || fwrite(flagged, sizeof(uint32_t), m, df) != m) status = 1;
    if (df) fclose(df);
    printf("flagged inputs (any tier, either kind): %llu\n", (unsigned long long)m);
    free(flagged);
  }
  return status;
}
