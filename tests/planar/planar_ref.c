/*
 * planar_ref.c -- see planar_ref.h.  TEST INFRASTRUCTURE; citations "file:line" are relative to the reference tree.
 */
#include "planar_ref.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ------------------------------------------------------------------ generators (the 3D mains' contract) */

static void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  /* Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11). */
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

static inline uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

static uint32_t xoshiro128pp_next(uint32_t s[4]) {   /* Blackman & Vigna, xoshiro128++ 1.0 */
  const uint32_t result = rotl32(s[0] + s[3], 7) + s[0], t = s[1] << 9;
  s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
  s[2] ^= t;
  s[3] = rotl32(s[3], 11);
  return result;
}

/* MWC64X (D. B. Thomas, 2011) as the LCG s' = A s mod M, s = c 2^32 + x, M = A 2^32 - 1 */
#define MWC_A 4294883355u
#define MWC_M 0xFFFEB81AFFFFFFFFull
static uint64_t mwc_mulmod(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % MWC_M); }
static uint64_t mwc_powmod(uint64_t g, uint64_t e) {
  uint64_t r = 1;
  for (; e; e >>= 1, g = mwc_mulmod(g, g))
    if (e & 1) r = mwc_mulmod(r, g);
  return r;
}

void planar_seed(const planar_params *P, uint64_t chain_id, uint32_t s[4]) {
  const uint32_t key[2] = {(uint32_t)P->seed, (uint32_t)(P->seed >> 32)};
  if (P->rng == PLANAR_RNG_XOSHIRO128PP) {
    const uint32_t ctr[4] = {(uint32_t)chain_id, (uint32_t)(chain_id >> 32), 0x5eedu, 0u};
    philox4x32_10(ctr, key, s);
    if ((s[0] | s[1] | s[2] | s[3]) == 0u) s[0] = 1u;
    return;
  }
  const uint32_t ctr[4] = {0u, 0u, 0x5eedu, 1u};
  uint32_t o[4];
  philox4x32_10(ctr, key, o);
  const uint64_t v = (uint64_t)o[0] | ((uint64_t)o[1] << 32);
  const uint64_t base = 1 + v % (MWC_M - 2);
  /* chain k starts k 2^40 outputs down the one sequence */
  const uint64_t st = mwc_mulmod(base, mwc_powmod(mwc_powmod(MWC_A, 1ull << 40), chain_id));
  s[0] = (uint32_t)st; s[1] = (uint32_t)(st >> 32); s[2] = 0u; s[3] = 0u;
}

uint32_t planar_next(int rng, uint32_t s[4]) {
  if (rng == PLANAR_RNG_XOSHIRO128PP) return xoshiro128pp_next(s);
  const uint32_t r = s[0] ^ s[1];
  const uint64_t t = (uint64_t)s[0] * MWC_A + s[1];
  s[0] = (uint32_t)t; s[1] = (uint32_t)(t >> 32);
  return r;
}

static inline double u01(uint32_t w) { return (double)(w >> 9) * (1.0 / 8388608.0); }

double planar_eps(int uniform_bits, uint32_t w_eps, uint32_t w_idx, uint32_t w_phi, uint32_t w_flip) {
  if (uniform_bits == 23) return u01(w_eps);
  const uint64_t lo = ((uint64_t)(w_phi & 511u) << 12) | ((uint64_t)(w_flip & 511u) << 3) | (uint64_t)(w_idx & 7u);
  return (double)(((uint64_t)w_eps << 21) | lo) * 0x1p-53;   /* < 2^53: exact */
}

/* where a uniform comes from: a chain's generator, or a list handed in by a hand check */
typedef struct {
  int rng;
  uint32_t *state;
  const double *u;
  int nu, used;
  int64_t words;
} source_t;

static uint32_t draw_w(source_t *s) { ++s->words; return planar_next(s->rng, s->state); }
static double draw_u(source_t *s) {
  if (s->state) return u01(draw_w(s));
  return s->used < s->nu ? s->u[s->used++] : 2.0;   /* the list ran out: the test fails, growth stops */
}

/* ------------------------------------------------------------------ the chain object, 2D/inc/eap_chain.jl:12-29 */

typedef struct {
  int64_t n;
  double *block;
  double *phi, *c, *s;   /* phis, cphis, sphis */
  double *nh, *mu, *xs;  /* 2 x n, column-major like the Julia matrices */
  double *us;
  double r[2], U;
} chain_t;

static int chain_alloc(chain_t *c, int64_t n) {
  c->n = n;
  c->block = (double *)calloc((size_t)(10 * n), sizeof(double));
  if (!c->block) return -1;
  c->phi = c->block; c->c = c->phi + n; c->s = c->c + n; c->us = c->s + n;
  c->nh = c->us + n; c->mu = c->nh + 2 * n; c->xs = c->mu + 2 * n;
  return 0;
}
static void chain_copy(chain_t *d, const chain_t *s) {   /* EAPChain(chain), :114-133: a deep copy */
  memcpy(d->block, s->block, sizeof(double) * (size_t)(10 * s->n));
  d->r[0] = s->r[0]; d->r[1] = s->r[1]; d->U = s->U;
}

static void dipole_cs(const planar_params *P, double c, double s, double mu[2]) {
  if (P->chain_type == PLANAR_DIELECTRIC) {   /* 2D/inc/dipole_response.jl:7-10 */
    const double a = (P->K1 - P->K2) * P->E0 * s;
    mu[0] = a * c + P->K2 * 0.0;
    mu[1] = a * s + P->K2 * P->E0;
  } else {                                    /* :25-27 with M = mu I, 2D/inc/eap_chain.jl:72 */
    mu[0] = P->mu * c + 0.0 * s;
    mu[1] = 0.0 * c + P->mu * s;
  }
}
void planar_dipole(const planar_params *P, double phi, double mu_out[2]) { dipole_cs(P, cos(phi), sin(phi), mu_out); }

static void set_monomer(const planar_params *P, chain_t *ch, int64_t i) {   /* :174-180 */
  ch->c[i] = cos(ch->phi[i]);
  ch->s[i] = sin(ch->phi[i]);
  ch->nh[2 * i] = ch->c[i]; ch->nh[2 * i + 1] = ch->s[i];   /* :33 */
  dipole_cs(P, ch->c[i], ch->s[i], ch->mu + 2 * i);
  ch->us[i] = -0.5 * P->E0 * ch->mu[2 * i + 1];             /* :64 */
}

static void update_xs(const planar_params *P, chain_t *ch) {   /* :49-51: b (cumsum(nh) - nh / 2) */
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = 0; i < ch->n; ++i) {
    a0 += ch->nh[2 * i]; a1 += ch->nh[2 * i + 1];
    ch->xs[2 * i] = P->b * (a0 - 0.5 * ch->nh[2 * i]);
    ch->xs[2 * i + 1] = P->b * (a1 - 0.5 * ch->nh[2 * i + 1]);
  }
}
static void end_to_end(const planar_params *P, chain_t *ch) {   /* :259-260 */
  const int64_t e = ch->n - 1;
  ch->r[0] = ch->xs[2 * e] + P->b / 2.0 * ch->nh[2 * e];
  ch->r[1] = ch->xs[2 * e + 1] + P->b / 2.0 * ch->nh[2 * e + 1];
}
static double pair_term(const double *xi, const double *xj, const double *mi, const double *mj) {   /* :141-148: the 3D kernel on 2-vectors */
  const double rx = xi[0] - xj[0], rz = xi[1] - xj[1];
  const double r2 = rx * rx + rz * rz, rmag = sqrt(r2);
  const double hx = rx / rmag, hz = rz / rmag, r3 = r2 * rmag;
  return ((mi[0] * mj[0] + mi[1] * mj[1]) - 3 * (mi[0] * hx + mi[1] * hz) * (mj[0] * hx + mj[1] * hz)) / (4 * M_PI * r3);
}
static double sum_us(const chain_t *ch) {
  double s = 0.0;
  for (int64_t i = 0; i < ch->n; ++i) s += ch->us[i];
  return s;
}
static double chain_U(const planar_params *P, const chain_t *ch) {   /* 2D/inc/energy.jl:7-23 */
  double U = sum_us(ch);
  if (P->energy_type == PLANAR_ISING) {                               /* :156-169 */
    double up = 0.0;
    for (int64_t i = 0; i + 1 < ch->n; ++i) up += pair_term(ch->xs + 2 * i, ch->xs + 2 * i + 2, ch->mu + 2 * i, ch->mu + 2 * i + 2);
    U += up;
  } else if (P->energy_type == PLANAR_INTERACTING) {                  /* :137-152 */
    double up = 0.0;
    for (int64_t i = 0; i < ch->n; ++i)
      for (int64_t j = i + 1; j < ch->n; ++j) up += pair_term(ch->xs + 2 * i, ch->xs + 2 * j, ch->mu + 2 * i, ch->mu + 2 * j);
    U += up;
  }
  return U - (ch->r[0] * P->Fx + ch->r[1] * P->Fz);
}
static void chain_derive(const planar_params *P, chain_t *ch) {   /* :103-110 */
  for (int64_t i = 0; i < ch->n; ++i) set_monomer(P, ch, i);
  update_xs(P, ch);
  end_to_end(P, ch);
  ch->U = chain_U(P, ch);
}
static void chain_move(const planar_params *P, chain_t *ch, int64_t idx, double dphi) {   /* move!, :171-186: phi is not wrapped */
  ch->phi[idx] += dphi;
  set_monomer(P, ch, idx);
  update_xs(P, ch);
  end_to_end(P, ch);
  ch->U = chain_U(P, ch);
}
static void chain_p(const chain_t *ch, double p[2]) {   /* chain_mu, :262 */
  p[0] = p[1] = 0.0;
  for (int64_t i = 0; i < ch->n; ++i) { p[0] += ch->mu[2 * i]; p[1] += ch->mu[2 * i + 1]; }
}

static double link_p(const chain_t *ch, int64_t i, int64_t j) {   /* pflip_linear, :192 */
  return (1 + (ch->nh[2 * i] * ch->nh[2 * j] + ch->nh[2 * i + 1] * ch->nh[2 * j + 1])) / 2;
}

/* cluster_flip!, :194-257, once the flip draw has said `flip` (the contract's order: planar_ref.h) */
static double cluster_flip(const planar_params *P, source_t *src, chain_t *ch, int64_t idx, int flip, int64_t *lower_out,
                           int64_t *upper_out, int64_t *tests) {
  *lower_out = *upper_out = idx;
  if (!flip) return 1.0;                                        /* :253-255 */
  const int64_t n = ch->n;
  double upper_p = 0.0, lower_p = 0.0;                          /* at a chain end: p = 0, no draw (:203-206,220-223) */
  int64_t upper = idx, lower = idx;
  int gu = upper < n - 1, gl = lower > 0;
  while (gu || gl) {                                            /* :199-230, the two ends interleaved */
    if (gu) {
      upper_p = link_p(ch, upper, upper + 1);
      ++*tests;
      if (draw_u(src) <= upper_p) { ++upper; if (upper >= n - 1) { upper_p = 0.0; gu = 0; } }
      else gu = 0;
    }
    if (gl) {
      lower_p = link_p(ch, lower, lower - 1);
      ++*tests;
      if (draw_u(src) <= lower_p) { --lower; if (lower <= 0) { lower_p = 0.0; gl = 0; } }
      else gl = 0;
    }
  }
  for (int64_t i = lower; i <= upper; ++i) chain_move(P, ch, i, M_PI);   /* flip_n!, :188-190,235-237 */
  const double new_upper_p = upper < n - 1 ? link_p(ch, upper, upper + 1) : 0.0;   /* :239-248 */
  const double new_lower_p = lower > 0 ? link_p(ch, lower, lower - 1) : 0.0;
  *lower_out = lower; *upper_out = upper;
  return ((1 - new_upper_p) * (1 - new_lower_p)) / ((1 - upper_p) * (1 - lower_p));   /* :249-252 */
}

/* AntiDipoleWeightFunction, 2D/inc/average.jl:104-124; WeightlessFunction is the constant 1.0 (:102) */
static double weight(const planar_params *P, const chain_t *ch) {
  if (!P->umbrella) return 1.0;
  const double lead = P->chain_type == PLANAR_DIELECTRIC ? (P->K1 + 2 * P->K2) * P->E0 * P->E0 : P->mu * P->E0;
  const double log_gauge = -lead * (double)P->n / (3 * P->kT);
  return sum_us(ch) / P->kT * (0.2 + 0.8 * exp(-(P->Fx * P->Fx + P->Fz * P->Fz) / P->kT)) - log_gauge;
}

static int check_params(const planar_params *P) {
  if (P->n < 1 || P->num_steps < 0) return -1;
  if (P->uniform_bits != 0 && P->uniform_bits != 23 && P->uniform_bits != 53) return -1;
  if (P->chain_type != PLANAR_DIELECTRIC && P->chain_type != PLANAR_POLAR) return -1;
  if (P->energy_type < 0 || P->energy_type > PLANAR_ISING) return -1;
  if (P->rng != PLANAR_RNG_MWC64X && P->rng != PLANAR_RNG_XOSHIRO128PP) return -1;
  return 0;
}

int planar_run(const planar_params *P, uint64_t chain_id, const double *phi0, const uint32_t *rng0, planar_result *out,
               double *final_phi) {
  if (check_params(P)) return -1;
  uint32_t state[4];
  source_t src = {P->rng, state, NULL, 0, 0, 0};
  chain_t cur, trial;
  if (chain_alloc(&cur, P->n)) return -2;
  if (chain_alloc(&trial, P->n)) { free(cur.block); return -2; }
  if (phi0) {
    memcpy(state, rng0, sizeof state);
    memcpy(cur.phi, phi0, sizeof(double) * (size_t)P->n);
  } else {                                                       /* EAPChain(pargs), :66-67 */
    planar_seed(P, chain_id, state);
    for (int64_t i = 0; i < P->n; ++i) cur.phi[i] = 6.28318530717958647692 * u01(draw_w(&src));
  }
  chain_derive(P, &cur);

  double phistep = P->phi_step;                                  /* 2D/mcmc_clustering_eap_chain.jl:149 */
  double logpi_prev = -cur.U / P->kT + weight(P, &cur);          /* Metropolis(chain, wf), 2D/inc/acceptance.jl:24-26 */
  double sum[PLANAR_NOBS], norm = 0.0;
  memset(sum, 0, sizeof sum);
  int64_t nacc = 0, natt = 0, nacc_total = 0, flips = 0, tests = 0;

  for (int64_t step = 1; step <= P->num_steps; ++step) {         /* :238 */
    const uint32_t w_idx = draw_w(&src), w_phi = draw_w(&src), w_flip = draw_w(&src);
    const int64_t idx = (int64_t)(((uint64_t)w_idx * (uint64_t)P->n) >> 32);   /* :239 */
    const double dphi = phistep * (2.0 * u01(w_phi) - 1.0);                      /* :240 */
    const int flip = u01(w_flip) <= P->cluster_prob;                             /* 2D/inc/eap_chain.jl:233 */
    flips += flip;
    chain_copy(&trial, &cur);                                                    /* :241 */
    chain_move(P, &trial, idx, dphi);                                            /* :242 */
    int64_t lo, up;
    const double alpha = cluster_flip(P, &src, &trial, idx, flip, &lo, &up, &tests);   /* :243 */
    const double eps = planar_eps(P->uniform_bits, draw_w(&src), w_idx, w_phi, w_flip);
    /* the Metropolis functor with alpha, 2D/inc/acceptance.jl:29-39: the cache keeps the accepted move's log(alpha) */
    const double logpi = -trial.U / P->kT + weight(P, &trial) + log(alpha);
    if ((logpi >= logpi_prev) || (eps < exp(logpi - logpi_prev))) {
      logpi_prev = logpi;
      chain_t tmp = cur; cur = trial; trial = tmp;                               /* :245 */
      ++nacc; ++nacc_total;
    }
    ++natt;
    if (P->adj_scale != 1.0 && P->steps_per_adjust > 0 && step % P->steps_per_adjust == 0) {   /* :257-275 */
      const double ar = (double)nacc / (double)natt;
      if (ar > P->adj_ub && phistep != M_PI) {
        nacc = 0; natt = 0;
        phistep = fmin(M_PI, phistep * P->adj_scale);
      } else if (ar < P->adj_lb) {
        nacc = 0; natt = 0;
        phistep /= P->adj_scale;
      }
    }
    /* record! x 8, :277-278; 2D/inc/average.jl:40-48,63-67 */
    double p[2];
    chain_p(&cur, p);
    const double r0 = cur.r[0], r1 = cur.r[1], U = cur.U;
    double v[PLANAR_NOBS];
    memset(v, 0, sizeof v);
    v[0] = r0; v[2] = r1; v[3] = r0 * r0; v[5] = r1 * r1; v[6] = r0 * r0 + r1 * r1;
    v[7] = p[0]; v[9] = p[1]; v[10] = p[0] * p[0]; v[12] = p[1] * p[1]; v[13] = p[0] * p[0] + p[1] * p[1];
    v[14] = U; v[15] = U * U;
    if (P->umbrella) {
      const double expw = exp(weight(P, &cur));
      for (int k = 0; k < PLANAR_NOBS; ++k) sum[k] += v[k] / expw;
      norm += 1.0 / expw;
    } else {
      for (int k = 0; k < PLANAR_NOBS; ++k) sum[k] += v[k];
      norm += 1;
    }
  }

  memcpy(out->sum, sum, sizeof sum);
  out->norm = norm;
  out->nacc_total = nacc_total;
  out->words = src.words;
  out->flips_proposed = flips;
  out->link_tests = tests;
  out->phi_step = phistep;
  out->r[0] = cur.r[0]; out->r[1] = cur.r[1];
  chain_p(&cur, out->p);
  out->U = cur.U;
  memcpy(out->rng, state, sizeof state);
  out->nacc_window = nacc; out->natt_window = natt;
  if (final_phi) memcpy(final_phi, cur.phi, sizeof(double) * (size_t)P->n);
  free(cur.block); free(trial.block);
  return 0;
}

double planar_energy(const planar_params *P, const double *phi, double r_out[2], double p_out[2], double *usum_out) {
  chain_t ch;
  if (chain_alloc(&ch, P->n)) return NAN;
  memcpy(ch.phi, phi, sizeof(double) * (size_t)P->n);
  chain_derive(P, &ch);
  if (r_out) { r_out[0] = ch.r[0]; r_out[1] = ch.r[1]; }
  if (p_out) chain_p(&ch, p_out);
  if (usum_out) *usum_out = sum_us(&ch);
  const double U = ch.U;
  free(ch.block);
  return U;
}

double planar_cluster_flip_u(const planar_params *P, double *phi, int64_t idx, const double *u, int nu, int64_t *lower,
                             int64_t *upper, int *flipped, int *used) {
  chain_t ch;
  if (chain_alloc(&ch, P->n)) return NAN;
  memcpy(ch.phi, phi, sizeof(double) * (size_t)P->n);
  chain_derive(P, &ch);
  source_t src = {P->rng, NULL, u, nu, 0, 0};
  const int flip = draw_u(&src) <= P->cluster_prob;
  int64_t tests = 0;
  const double alpha = cluster_flip(P, &src, &ch, idx, flip, lower, upper, &tests);
  memcpy(phi, ch.phi, sizeof(double) * (size_t)P->n);
  *flipped = flip;
  *used = src.used;
  free(ch.block);
  return alpha;
}
