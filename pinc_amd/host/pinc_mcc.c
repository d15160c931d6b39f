/*
 * pinc_mcc.c -- Monte Carlo collisions with a neutral background (host side,
 * C; an extension, the reference has no collision module).
 *
 *   mccAlloc     the ini's [collisions] section, validated
 *   mccCollide   one pinc_hip_collide per species with a non-zero rate
 *   mccCounts    cumulative elastic / charge-exchange counts
 *   mccIonize    one pinc_hip_ionize per species with an ionisation rate; the
 *                species that grew are taken in as puMigrate takes immigrants
 *   mccIonizations  cumulative births per projectile species
 *   mccCoulomb   one pinc_hip_coulomb per species pair with a Coulomb logarithm
 *   mccCoulombCoef, mccCoulombCounts  a pair's coefficient K_ab and its
 *                cumulative collisions
 *
 * The rules are pinc_hip_collide's, pinc_hip_ionize's and pinc_hip_coulomb's
 * (include/pinc_hip.h).
 */
#define _GNU_SOURCE
#include "pinc_internal.h"
#include <math.h>

struct Collisions {
	int nSpecies, nDims;
	int active[PINC_MAX_SPECIES];        /* a rate of the species is not zero */
	pinc_collide_t par[PINC_MAX_SPECIES]; /* key set per launch */
	unsigned long long seed, step;
	unsigned long long *counts;           /* device: [s][2] */
	/* ionisation: its own call counter, so that mccCollide's draws do not
	 * depend on whether ionisation runs */
	int ionActive[PINC_MAX_SPECIES];      /* an ionisation rate of the species is not zero */
	pinc_ionize_t ion[PINC_MAX_SPECIES];  /* key set per launch */
	unsigned long long ionStep;
	unsigned long long births[PINC_MAX_SPECIES]; /* host: cumulative, per projectile */
	unsigned long long *ionRes;           /* device: [s][2], births and the overflow word */
	int *ionWork;                         /* device scratch of pinc_hip_ionize */
	long ionWorkInts;
	/* Coulomb collisions between the species: again a call counter of their
	 * own, so that neither of the streams above depends on them */
	int couAny;
	double couK[PINC_MAX_SPECIES][PINC_MAX_SPECIES];  /* K_ab, a <= b; 0: the pair is off */
	double couFrac[PINC_MAX_SPECIES][PINC_MAX_SPECIES]; /* [a][b] = mu_ab / m_a */
	double couH[3];
	unsigned long long couStep;
	unsigned long long *couCounts;        /* device: [a][b] */
	int *couWork;                         /* device scratch of pinc_hip_coulomb */
	long couWorkInts;
};

static const char *const kRateKeys[4] = {"collisions:elasticNu", "collisions:cexNu", "collisions:elasticSigma",
                                         "collisions:cexSigma"};

/* per-species values of a rate key (zeros if the key is missing) */
static double *rate_arr(const dictionary *ini, const char *key, int ns) {
	if (!iniHas(ini, key)) return calloc(ns, sizeof(double));
	const int n = iniGetNElements(ini, key);
	if (n != ns) msg(ERROR, "%s takes one value per species (%d), not %d", key, ns, n);
	double *a = iniGetDoubleArr(ini, key, ns);
	for (int s = 0; s < ns; s++)
		if (!(a[s] >= 0.0) || !isfinite(a[s])) msg(ERROR, "%s must be >= 0 and finite (species %d: %g)", key, s, a[s]);
	return a;
}

/* uAlloc rewrites population:mass (SI, then computational particles of
 * normalised mass): the neutral's share of the pair mass b = m_n / (m_s + m_n)
 * is taken from the input's own values before that (pinc_core.c calls this at
 * the top of uAlloc) and kept in the ini for mccAlloc */
void pinc_mcc_mass_fraction(dictionary *ini) {
	/* the derived key is this library's own: an input that sets it would
	 * override the masses without a word */
	if (iniHas(ini, "collisions:neutralMassFraction"))
		msg(ERROR, "collisions:neutralMassFraction is derived from collisions:neutralMass and population:mass; "
		           "it cannot be set in the input");
	if (iniHas(ini, "collisions:macroWeight"))
		msg(ERROR, "collisions:macroWeight is derived from population:density and population:nParticles; "
		           "it cannot be set in the input");
	if (!iniHas(ini, "collisions:neutralMass")) return;
	const int ns = iniGetInt(ini, "population:nSpecies");
	const double mn = iniGetDouble(ini, "collisions:neutralMass");
	if (!(mn > 0.0) || !isfinite(mn)) msg(ERROR, "collisions:neutralMass must be > 0 and finite, not %g", mn);
	double *m = iniGetDoubleArr(ini, "population:mass", ns);
	double b[PINC_MAX_SPECIES] = {0};
	for (int s = 0; s < ns && s < PINC_MAX_SPECIES; s++) b[s] = mn / (m[s] + mn);
	iniSetDoubleArr(ini, "collisions:neutralMassFraction", b, ns < PINC_MAX_SPECIES ? ns : PINC_MAX_SPECIES);
	free(m);
}

/* The Coulomb coefficient needs the real particles per computational particle,
 * which the normalised ini no longer shows (uNormalize folds them into charge
 * and mass): uAlloc leaves its Units' weights here for mccAlloc */
void pinc_mcc_macro_weight(dictionary *ini, const double *weights, int ns) {
	if (!iniHas(ini, "collisions:coulombLog")) return;
	iniSetDoubleArr(ini, "collisions:macroWeight", weights, ns < PINC_MAX_SPECIES ? ns : PINC_MAX_SPECIES);
}

/* collisions:coulombLog, validated: ln Lambda per pair, row-major (zeros if
 * the key is missing); *present says whether it is there */
static double *coulomb_log(const dictionary *ini, int ns, int nd, int *present) {
	*present = iniHas(ini, "collisions:coulombLog");
	if (!*present) return calloc((size_t)ns * ns, sizeof(double));
	if (nd != 3) msg(ERROR, "collisions:coulombLog needs grid:nDims = 3 (the scattering has three velocity components), not %d", nd);
	const int n = iniGetNElements(ini, "collisions:coulombLog");
	if (n != ns * ns)
		msg(ERROR, "collisions:coulombLog takes nSpecies x nSpecies values (%d, row-major), not %d", ns * ns, n);
	double *L = iniGetDoubleArr(ini, "collisions:coulombLog", ns * ns);
	for (int a = 0; a < ns; a++)
		for (int b = 0; b < ns; b++) {
			if (!(L[a * ns + b] >= 0.0) || !isfinite(L[a * ns + b]))
				msg(ERROR, "collisions:coulombLog must be >= 0 and finite (pair %d, %d: %g)", a, b, L[a * ns + b]);
			if (L[a * ns + b] != L[b * ns + a])
				msg(ERROR, "collisions:coulombLog must be symmetric (pair %d, %d: %g against %g)", a, b, L[a * ns + b],
				    L[b * ns + a]);
		}
	return L;
}

Collisions *mccAlloc(const dictionary *ini, const Population *pop, const MpiInfo *mpiInfo) {
	(void)mpiInfo;
	const int ns = pop->nSpecies, nd = pop->nDims;
	static const char *const known[15] = {"elasticNu", "cexNu", "elasticSigma", "cexSigma", "neutralMass", "neutralVth",
	                                      "neutralDrift", "seed", "neutralMassFraction", "ionNu", "ionSigma",
	                                      "ionThreshold", "ionSpecies", "coulombLog", "macroWeight"};
	int present = 0;
	const char *unknown = pinc_ini_unknown_key(ini, "collisions", known, 15, &present);
	if (!present) return NULL;
	if (unknown)
		msg(ERROR, "%s is no key of [collisions] (elasticNu, cexNu, elasticSigma, cexSigma, neutralMass, neutralVth, "
		           "neutralDrift, seed, ionNu, ionSigma, ionThreshold, ionSpecies, coulombLog)", unknown);
	if (ns > PINC_MAX_SPECIES) msg(ERROR, "collisions: more than %d species", PINC_MAX_SPECIES);

	double *rate[4];
	for (int k = 0; k < 4; k++) rate[k] = rate_arr(ini, kRateKeys[k], ns);
	/* ionisation: rates, the threshold speed (rate_arr's rules: one value per
	 * species, >= 0, finite) and the species that receives the ions */
	double *ionNu = rate_arr(ini, "collisions:ionNu", ns), *ionSig = rate_arr(ini, "collisions:ionSigma", ns);
	double *ionWth = rate_arr(ini, "collisions:ionThreshold", ns);
	int ionTarget[PINC_MAX_SPECIES] = {0}, anyIon = 0;
	for (int s = 0; s < ns; s++) anyIon |= ionNu[s] > 0 || ionSig[s] > 0;
	if (anyIon) {
		if (!iniHas(ini, "collisions:ionSpecies"))
			msg(ERROR, "collisions:ionSpecies (the species that receives the ions, one value per species) is required "
			           "with an ionisation rate");
		const int n = iniGetNElements(ini, "collisions:ionSpecies");
		if (n != ns) msg(ERROR, "collisions:ionSpecies takes one value per species (%d), not %d", ns, n);
		int *t = iniGetIntArr(ini, "collisions:ionSpecies", ns);
		for (int s = 0; s < ns; s++) {
			if (!(ionNu[s] > 0 || ionSig[s] > 0)) continue;
			if (t[s] < 0 || t[s] >= ns)
				msg(ERROR, "collisions:ionSpecies of species %d is %d: no species (0..%d)", s, t[s], ns - 1);
			if (t[s] == s)
				msg(ERROR, "collisions:ionSpecies of species %d is the projectile itself: the ions need another species", s);
			ionTarget[s] = t[s];
		}
		free(t);
	}
	double vth = iniHas(ini, "collisions:neutralVth") ? iniGetDouble(ini, "collisions:neutralVth") : 0.0;
	if (!(vth >= 0.0) || !isfinite(vth)) msg(ERROR, "collisions:neutralVth must be >= 0 and finite, not %g", vth);
	double drift[3] = {0, 0, 0};
	if (iniHas(ini, "collisions:neutralDrift")) {
		const int n = iniGetNElements(ini, "collisions:neutralDrift");
		if (n != nd) msg(ERROR, "collisions:neutralDrift takes one value per dimension (%d), not %d", nd, n);
		double *a = iniGetDoubleArr(ini, "collisions:neutralDrift", nd);
		for (int d = 0; d < nd; d++) {
			if (!isfinite(a[d])) msg(ERROR, "collisions:neutralDrift must be finite");
			drift[d] = a[d];
		}
		free(a);
	}
	/* Coulomb collisions: K_ab of every pair with a logarithm (DESIGN.md section 4,
	 * "Coulomb collisions"), from the normalised charges and masses, the real
	 * particles per computational particle W and the cell volume in stepSize[0]^3 */
	int couPresent = 0, anyCou = 0;
	double *couLog = coulomb_log(ini, ns, nd, &couPresent);
	double couK[PINC_MAX_SPECIES][PINC_MAX_SPECIES] = {{0}}, couFrac[PINC_MAX_SPECIES][PINC_MAX_SPECIES] = {{0}};
	for (int k = 0; k < ns * ns; k++) anyCou |= couLog[k] > 0;
	if (anyCou) {
		if (!iniHas(ini, "collisions:macroWeight"))
			msg(ERROR, "collisions:coulombLog needs the particle weights of uAlloc (collisions:macroWeight is missing)");
		double *W = iniGetDoubleArr(ini, "collisions:macroWeight", ns);
		double *q = iniGetDoubleArr(ini, "population:charge", ns), *m = iniGetDoubleArr(ini, "population:mass", ns);
		double *step = iniGetDoubleArr(ini, "grid:stepSize", nd);
		const double cellVol = (step[1] / step[0]) * (step[2] / step[0]);
		for (int a = 0; a < ns; a++)
			for (int b = a; b < ns; b++) {
				if (!(couLog[a * ns + b] > 0)) continue;
				if (a != b && fabs(W[a] - W[b]) > 1e-12 * fabs(W[a]))
					msg(ERROR, "collisions:coulombLog of the pair %d, %d: the species stand for %g and %g real particles "
					           "per computational particle; unlike pairs need equal weights", a, b, W[a], W[b]);
				if (!(m[a] > 0) || !(m[b] > 0) || !(W[a] > 0))
					msg(ERROR, "collisions:coulombLog of the pair %d, %d: masses and weights must be > 0", a, b);
				const double mu = m[a] * m[b] / (m[a] + m[b]), qq = q[a] * q[b] / mu;
				couK[a][b] = qq * qq * couLog[a * ns + b] / (8.0 * M_PI * W[a] * cellVol);
				couFrac[a][b] = mu / m[a];
				couFrac[b][a] = mu / m[b];
				if (!isfinite(couK[a][b])) msg(ERROR, "collisions:coulombLog of the pair %d, %d: K is not finite", a, b);
			}
		free(W);
		free(q);
		free(m);
		free(step);
	}
	free(couLog);
	int anyElastic = 0, any = anyIon || anyCou;
	for (int s = 0; s < ns; s++) {
		anyElastic |= rate[0][s] > 0 || rate[2][s] > 0;
		any |= rate[0][s] > 0 || rate[1][s] > 0 || rate[2][s] > 0 || rate[3][s] > 0;
	}
	double b[PINC_MAX_SPECIES] = {0};
	if (iniHas(ini, "collisions:neutralMass")) {
		const double mn = iniGetDouble(ini, "collisions:neutralMass");
		if (!(mn > 0.0) || !isfinite(mn)) msg(ERROR, "collisions:neutralMass must be > 0 and finite, not %g", mn);
		if (iniHas(ini, "collisions:neutralMassFraction")) {
			double *f = iniGetDoubleArr(ini, "collisions:neutralMassFraction", ns);
			for (int s = 0; s < ns; s++) b[s] = f[s];
			free(f);
		} else {
			/* an ini that uAlloc has not rewritten: the masses as they stand */
			double *m = iniGetDoubleArr(ini, "population:mass", ns);
			for (int s = 0; s < ns; s++) b[s] = mn / (m[s] + mn);
			free(m);
		}
	} else if (anyElastic) {
		msg(ERROR, "collisions:neutralMass is required with an elastic rate");
	}
	Collisions *C = NULL;
	if (any) {
		double *step = iniGetDoubleArr(ini, "grid:stepSize", nd);
		C = calloc(1, sizeof(*C));
		C->nSpecies = ns;
		C->nDims = nd;
		C->seed = iniHas(ini, "collisions:seed") ? (unsigned long long)iniGetLongInt(ini, "collisions:seed") : 0ULL;
		for (int s = 0; s < ns; s++) {
			pinc_collide_t *p = &C->par[s];
			p->nu[0] = rate[0][s];
			p->nu[1] = rate[1][s];
			p->sig[0] = rate[2][s];
			p->sig[1] = rate[3][s];
			p->b = b[s];
			p->vth = vth;
			for (int d = 0; d < 3; d++) {
				p->drift[d] = drift[d];
				p->h[d] = d < nd ? step[d] / step[0] : 1.0;
			}
			C->active[s] = p->nu[0] > 0 || p->nu[1] > 0 || p->sig[0] > 0 || p->sig[1] > 0;
			pinc_ionize_t *q = &C->ion[s];
			q->nu = ionNu[s];
			q->sig = ionSig[s];
			q->wth = ionWth[s];
			q->vth = vth;
			for (int d = 0; d < 3; d++) {
				q->drift[d] = p->drift[d];
				q->h[d] = p->h[d];
			}
			q->target = ionTarget[s];
			C->ionActive[s] = q->nu > 0 || q->sig > 0;
		}
		C->couAny = anyCou;
		for (int a = 0; a < ns; a++)
			for (int b = 0; b < ns; b++) {
				C->couK[a][b] = couK[a][b];
				C->couFrac[a][b] = couFrac[a][b];
			}
		for (int d = 0; d < 3; d++) C->couH[d] = d < nd ? step[d] / step[0] : 1.0;
		free(step);
		pinc_ctx_require();
		pinc_check(pinc_hip_malloc((void **)&C->counts, 2 * PINC_MAX_SPECIES * sizeof(unsigned long long)),
		           "collision counters");
		pinc_check(pinc_hip_memset(C->counts, 0, 2 * PINC_MAX_SPECIES * sizeof(unsigned long long), g_pinc.stream),
		           "collision counters");
		if (anyIon) {
			pinc_check(pinc_hip_malloc((void **)&C->ionRes, 2 * PINC_MAX_SPECIES * sizeof(unsigned long long)),
			           "ionisation counters");
			pinc_check(pinc_hip_memset(C->ionRes, 0, 2 * PINC_MAX_SPECIES * sizeof(unsigned long long), g_pinc.stream),
			           "ionisation counters");
		}
		if (anyCou) {
			const unsigned long bytes = PINC_MAX_SPECIES * PINC_MAX_SPECIES * sizeof(unsigned long long);
			pinc_check(pinc_hip_malloc((void **)&C->couCounts, bytes), "Coulomb counters");
			pinc_check(pinc_hip_memset(C->couCounts, 0, bytes, g_pinc.stream), "Coulomb counters");
		}
	}
	for (int k = 0; k < 4; k++) free(rate[k]);
	free(ionNu);
	free(ionSig);
	free(ionWth);
	return C;
}

void mccCollide(Collisions *C, Population *pop) {
	if (!C) return;
	pinc_pop_flush_host(pop);
	PincDevPop *dv = pop->dev;
	if (dv->pending)
		msg(ERROR, "mccCollide with a fused puAcc's move pending: collide the settled velocities, after puMove");
	pinc_pop_t p = pinc_devpop(pop);
	for (int s = 0; s < C->nSpecies; s++) {
		if (!C->active[s]) continue;
		pinc_collide_t par = C->par[s];
		par.key = pinc_hip_collide_key(C->seed, C->step, g_pinc.rank, s);
		pinc_check(pinc_hip_collide(p, s, p.v, par, C->counts + 2 * s, g_pinc.stream), "collide");
		/* a collider's new velocity (a fast neutral's, in charge exchange) is
		 * held to population:maxVel now, not at the next kick: the assert
		 * word is read by the step's pPosAssertInLocalFrame */
		if (isfinite(g_pinc.maxVel)) {
			pinc_check(pinc_hip_vel_assert(p, s, g_pinc.maxVel, g_pinc.dErr, g_pinc.stream), "collide: maxVel");
			g_pinc.errSerial++;
		}
	}
	C->step++;
	/* (pinc_pop_flush_host left the device arrays the truth: pSyncToHost reads them) */
}

/* species q grew by `births` at its tail: what puMigrate does after
 * puMigrateImport (pinc_pusher.c).  The new slots' flags are not written, as
 * an import leaves them; depEnd and cellValid stay, so that distr deposits the
 * tail [depEnd, iStop) as it deposits immigrants */
static void take_in_births(Population *pop, int q, long births) {
	PincDevPop *dv = pop->dev;
	const long before = pop->iStop[q] - pop->iStart[q];
	pop->iStop[q] += births;
	if (dv->sorted && dv->cntValid[q]) {
		pinc_pop_t p = pinc_devpop(pop);
		pinc_check(pinc_hip_count_keys(p, q, before, dv->geom, dv->tileWidth, dv->keyCnt[q], g_pinc.stream),
		           "count the keys of the born");
	}
	dv->flagsValid = 0;
}

void mccIonize(Collisions *C, Population *pop) {
	if (!C || !C->ionRes) return;
	pinc_pop_flush_host(pop);
	PincDevPop *dv = pop->dev;
	if (dv->pending)
		msg(ERROR, "mccIonize with a fused puAcc's move pending: ionise the settled particles, after puMigrate");
	for (int s = 0; s < C->nSpecies; s++) {
		if (!C->ionActive[s]) continue;
		pinc_ionize_t par = C->ion[s];
		const int t = par.target;
		par.key = pinc_hip_ionize_key(C->seed, C->ionStep, g_pinc.rank, s);
		pinc_pop_t p = pinc_devpop(pop);
		const long need = pinc_hip_ionize_work(p.iStop[s] - p.iStart[s]);
		if (need > C->ionWorkInts) {
			pinc_check(pinc_hip_stream_sync(g_pinc.stream), "ionisation scratch");
			pinc_hip_free(C->ionWork);
			C->ionWorkInts = need + need / 4;
			pinc_check(pinc_hip_malloc((void **)&C->ionWork, C->ionWorkInts * sizeof(int)), "ionisation scratch");
		}
		pinc_check(pinc_hip_ionize(p, s, par, C->ionWork, C->ionWorkInts, C->ionRes + 2 * s, g_pinc.stream), "ionize");
		unsigned long long res[2];
		pinc_check(pinc_hip_d2h(res, C->ionRes + 2 * s, sizeof(res), g_pinc.stream), "ionisation counters");
		if (res[1]) {
			const int q = pop->iStart[s + 1] - pop->iStop[s] <= pop->iStart[t + 1] - pop->iStop[t] ? s : t;
			msg(ERROR, "ionisation: allocated only %li particles of specie %i", pop->iStart[q + 1] - pop->iStart[q], q);
		}
		const long births = (long)(res[0] - C->births[s]);
		C->births[s] = res[0];
		if (births) {
			take_in_births(pop, s, births);
			take_in_births(pop, t, births);
		}
		/* the electrons' new velocities are held to population:maxVel now, as
		 * mccCollide's are (the born electrons are in the range by now) */
		if (isfinite(g_pinc.maxVel)) {
			pinc_check(pinc_hip_vel_assert(pinc_devpop(pop), s, g_pinc.maxVel, g_pinc.dErr, g_pinc.stream),
			           "ionize: maxVel");
			g_pinc.errSerial++;
		}
	}
	C->ionStep++;
}

int mccCoulombActive(const Collisions *C) { return C && C->couAny; }

void mccCoulomb(Collisions *C, Population *pop) {
	if (!C || !C->couAny) return;
	pinc_pop_flush_host(pop);
	PincDevPop *dv = pop->dev;
	if (dv->pending)
		msg(ERROR, "mccCoulomb with a fused puAcc's move pending: collide the settled particles, after puMigrate");
	const pinc_pop_t p = pinc_devpop(pop);
	const pinc_geom_t g = dv->geom;
	const long nCells = (long)g.T[0] * g.T[1] * g.nloc;
	int touched[PINC_MAX_SPECIES] = {0};
	for (int a = 0; a < C->nSpecies; a++)
		for (int b = a; b < C->nSpecies; b++) {
			if (!(C->couK[a][b] > 0)) continue;
			pinc_coulomb_t par = {.K = C->couK[a][b], .fa = C->couFrac[a][b], .fb = C->couFrac[b][a]};
			for (int d = 0; d < 3; d++) par.h[d] = C->couH[d];
			par.key = pinc_hip_coulomb_key(C->seed, C->couStep, g_pinc.rank, a, b);
			const long need = pinc_hip_coulomb_work(p.iStop[a] - p.iStart[a], a == b ? 0 : p.iStop[b] - p.iStart[b], nCells);
			if (need > C->couWorkInts) {
				pinc_check(pinc_hip_stream_sync(g_pinc.stream), "Coulomb scratch");
				pinc_hip_free(C->couWork);
				C->couWorkInts = need + need / 4;
				pinc_check(pinc_hip_malloc((void **)&C->couWork, C->couWorkInts * sizeof(int)), "Coulomb scratch");
			}
			pinc_check(pinc_hip_coulomb(p, a, b, g, par, C->couWork, C->couWorkInts,
			                            C->couCounts + a * PINC_MAX_SPECIES + b, g_pinc.stream), "coulomb");
			touched[a] = touched[b] = 1;
		}
	/* The in-push sort keys a particle by the cell of x + v (pinc_hip_count_keys),
	 * and a counting push has counted those keys with the velocities it left.
	 * A scattered velocity may take x + v to another brick, so the counts of a
	 * touched species no longer reserve what the sorting push will place: it
	 * counts again (pinc_pusher.c, as after pinc_obj.c's removals) */
	if (dv->sorted)
		for (int s = 0; s < C->nSpecies; s++)
			if (touched[s]) dv->cntValid[s] = 0;
	/* the scattered velocities are held to population:maxVel now, as mccCollide's are */
	if (isfinite(g_pinc.maxVel))
		for (int s = 0; s < C->nSpecies; s++) {
			if (!touched[s]) continue;
			pinc_check(pinc_hip_vel_assert(p, s, g_pinc.maxVel, g_pinc.dErr, g_pinc.stream), "coulomb: maxVel");
			g_pinc.errSerial++;
		}
	C->couStep++;
}

static void coulomb_pair(const Collisions *C, const char *who, int *a, int *b) {
	if (*a < 0 || *a >= C->nSpecies || *b < 0 || *b >= C->nSpecies) msg(ERROR, "%s: pair %d, %d out of range", who, *a, *b);
	if (*a > *b) {
		const int t = *a;
		*a = *b;
		*b = t;
	}
}

double mccCoulombCoef(const Collisions *C, int a, int b) {
	if (!C) return 0.0;
	coulomb_pair(C, "mccCoulombCoef", &a, &b);
	return C->couK[a][b];
}

unsigned long long mccCoulombCounts(const Collisions *C, int a, int b) {
	if (!C || !C->couCounts) return 0;
	coulomb_pair(C, "mccCoulombCounts", &a, &b);
	unsigned long long n = 0;
	pinc_check(pinc_hip_d2h(&n, C->couCounts + a * PINC_MAX_SPECIES + b, sizeof(n), g_pinc.stream), "Coulomb counters");
	return n;
}

unsigned long long mccIonizations(const Collisions *C, int s) {
	if (!C) return 0;
	if (s < 0 || s >= C->nSpecies) msg(ERROR, "mccIonizations: species %d out of range", s);
	return C->births[s];
}

void mccCounts(const Collisions *C, int s, unsigned long long out[2]) {
	out[0] = out[1] = 0;
	if (!C) return;
	if (s < 0 || s >= C->nSpecies) msg(ERROR, "mccCounts: species %d out of range", s);
	pinc_check(pinc_hip_d2h(out, C->counts + 2 * s, 2 * sizeof(unsigned long long), g_pinc.stream), "collision counters");
}

void mccFree(Collisions *C) {
	if (!C) return;
	pinc_hip_free(C->counts);
	pinc_hip_free(C->ionRes);
	pinc_hip_free(C->ionWork);
	pinc_hip_free(C->couCounts);
	pinc_hip_free(C->couWork);
	free(C);
}
