/*
 * pinc_twopop.c -- a C caller of libpinc.so with TWO populations in one world
 * (TEST DRIVER, ADVICE r06 "medium"): one set of grids (rho, phi, E), one
 * neighbourhood, populations A and B that kick with the same E.  It drives
 * the host state that lives outside a population once a second one exists:
 * the E grid's cache of every species' rescaled E (filled by each fused push
 * from the pushing population's q/m), the registry of pending pushes that a
 * grid write walks, and what pFree takes out of it.
 *
 *   pinc_twopop <A.ini> <B.ini> <outDir> [section:key=value ...]
 *
 * The two files differ in their population: section only; the overrides go to
 * both dictionaries.  Keys the driver reads itself (from A's dictionary):
 *   twopop:scenario   alone | read | drop | ewrite | move | free | bonly | nine
 *   twopop:then       read | drop | ewrite: what follows the push in alone
 *                     and bonly (default read)
 *   twopop:seedA, twopop:seedB   seeds of the Maxwellians (default 11, 23)
 *
 * Both populations start on their lattice with Maxwellian velocities; A's
 * species 0 is displaced in one octant of the box (lattice_maxwell below), so
 * that E, from A's charge by distr, solve and the finite difference, is not
 * zero.  A's puAcc(A, E) comes first in every scenario but bonly; with a tiled, fused
 * population and sortInterval = 1 it is a sorting push whose move stays
 * pending.  Then:
 *   alone    nothing (B is never pushed), then twopop:then
 *   read     puAcc(B, E); the populations are read (pSyncToHost)
 *   drop     puAcc(B, E); A's extract without a move
 *   ewrite   puAcc(B, E); gMul(E, 2.0) as main.c:183-185
 *   move     puAcc(B, E); puMove(A): the committed kick
 *   free     puAcc(B, E); pFree(A); gMul(E, 2.0): only B is left
 *   bonly    puAcc(B, E) alone (A is never pushed), then twopop:then
 *   nine     A and eight more populations of A's dictionary each run a
 *            sorting puAcc: the ninth ends the run in msg(ERROR)
 *
 * Output: "TWOPOP: qm <A|B> <s> <q/m>" per species (normalised), and in
 * <outDir> raw little-endian float64 files <A|B>_<init|end>_s<s>_<pos|vel>.f64
 * of n x nDims values each: the state after the initialisation and the
 * observable state at the end of the scenario.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/select.h>   /* before pinc.h, which defines the select() macro */
#include "pinc.h"

static void dump(Population *pop, const char *dir, const char *who, const char *when) {
	pSyncToHost(pop);
	int nd = pop->nDims;
	for (int s = 0; s < pop->nSpecies; s++) {
		long a = pop->iStart[s], n = pop->iStop[s] - a;
		const double *src[2] = {pop->pos + a * nd, pop->vel + a * nd};
		const char *what[2] = {"pos", "vel"};
		for (int k = 0; k < 2; k++) {
			char path[2048];
			snprintf(path, sizeof(path), "%s/%s_%s_s%d_%s.f64", dir, who, when, s, what[k]);
			FILE *f = fopen(path, "wb");
			if (!f || fwrite(src[k], sizeof(double), (size_t)(n * nd), f) != (size_t)(n * nd) || fclose(f))
				msg(ERROR, "cannot write %s", path);
		}
	}
}

/* Lattice positions and Maxwellian velocities.  Species of equal counts share
 * their lattice sites, so with opposite charges the plasma is neutral node by
 * node, E is exactly zero and no kick would be seen.  With shift, species 0's
 * particles in the lower half of every dimension (global frame) are displaced
 * by shift cells along each: surface charge on that box's faces, a field with
 * all three components.  The lattice sits on multiples of 2^-9 cells, and with
 * a shift of 0.25 it still does: every deposit sum is then exact in fp64, so
 * rho, phi and E are the same bit for bit in every run, whatever the order of
 * the deposit's atomic adds. */
static void lattice_maxwell(dictionary *ini, Population *pop, const MpiInfo *mpiInfo, unsigned long long seed,
                            double shift) {
	pPosLattice(ini, pop, mpiInfo);
	if (shift != 0.) {
		int nd = pop->nDims;
		int *trueSize = iniGetIntArr(ini, "grid:trueSize", nd);
		int *nSub = iniGetIntArr(ini, "grid:nSubdomains", nd);
		pToGlobalFrame(pop, mpiInfo);
		for (long i = pop->iStart[0]; i < pop->iStop[0]; i++) {
			int inside = 1;
			for (int d = 0; d < nd; d++) inside &= pop->pos[i * nd + d] < 0.5 * trueSize[d] * nSub[d];
			for (int d = 0; d < nd && inside; d++) pop->pos[i * nd + d] += shift;
		}
		pToLocalFrame(pop, mpiInfo);
		free(trueSize);
		free(nSub);
	}
	pVelMaxwell(ini, pop, seed);
	pSyncToDevice(pop);
}

static dictionary *open_with(char *prog, char *file, int nOver, char **over) {
	char **av = malloc((nOver + 2) * sizeof(char *));
	av[0] = prog;
	av[1] = file;
	for (int i = 0; i < nOver; i++) av[2 + i] = over[i];
	dictionary *ini = iniOpen(nOver + 2, av);
	free(av);
	return ini;
}

int main(int argc, char *argv[]) {
	if (argc < 4) msg(ERROR, "usage: pinc_twopop <A.ini> <B.ini> <outDir> [section:key=value ...]");
	const char *dir = argv[3];
	dictionary *iniA = open_with(argv[0], argv[1], argc - 4, argv + 4);
	dictionary *iniB = open_with(argv[0], argv[2], argc - 4, argv + 4);
	char *scenario = iniGetStr(iniA, "twopop:scenario");
	char *thenKey = iniHas(iniA, "twopop:then") ? iniGetStr(iniA, "twopop:then") : NULL;
	unsigned long long seedA = iniHas(iniA, "twopop:seedA") ? (unsigned long long)iniGetLongInt(iniA, "twopop:seedA") : 11;
	unsigned long long seedB = iniHas(iniA, "twopop:seedB") ? (unsigned long long)iniGetLongInt(iniA, "twopop:seedB") : 23;
	const int alone = !strcmp(scenario, "alone"), bonly = !strcmp(scenario, "bonly"), nine = !strcmp(scenario, "nine");
	/* what follows the pushes: the scenario's own name, or twopop:then */
	const char *then = (alone || bonly) ? (thenKey ? thenKey : "read") : scenario;
	if (alone || bonly) {
		if (strcmp(then, "read") && strcmp(then, "ewrite") && (bonly || strcmp(then, "drop")))
			msg(ERROR, "twopop:then %s is none of read drop ewrite (bonly: read ewrite)", then);
	} else if (strcmp(scenario, "read") && strcmp(scenario, "drop") && strcmp(scenario, "ewrite") &&
	           strcmp(scenario, "move") && strcmp(scenario, "free") && !nine) {
		msg(ERROR, "twopop:scenario %s is none of alone read drop ewrite move free bonly nine", scenario);
	}

	void (*acc)(Population *, Grid *) =
	    (void (*)(Population *, Grid *))select(iniA, "methods:acc", puAcc3D1_set, puAcc3D1KE_set, puAccND1_set, puAccND1KE_set);
	void (*distr)(const Population *, Grid *) =
	    (void (*)(const Population *, Grid *))select(iniA, "methods:distr", puDistr3D1_set, puDistrND1_set);
	void (*extractEmigrants)(Population *, MpiInfo *) = (void (*)(Population *, MpiInfo *))select(
	    iniA, "methods:migrate", puExtractEmigrants3D_set, puExtractEmigrantsND_set);
	void (*solverInterface)() = select(iniA, "methods:poisson", mgSolver_set);
	void (*solve)() = NULL;
	void *(*solverAlloc)() = NULL;
	void (*solverFree)() = NULL;
	((void (*)(void (**)(), void *(**)(), void (**)()))solverInterface)(&solve, &solverAlloc, &solverFree);

	/* one world: the grids and the neighbourhood come from A's dictionary */
	Units *unitsA = uAlloc(iniA);
	uNormalize(iniA, unitsA);
	Units *unitsB = uAlloc(iniB);
	uNormalize(iniB, unitsB);
	MpiInfo *mpiInfo = gAllocMpi(iniA);
	Population *A = pAlloc(iniA);
	Population *B = pAlloc(iniB);
	Grid *E = gAlloc(iniA, VECTOR);
	Grid *rho = gAlloc(iniA, SCALAR);
	Grid *phi = gAlloc(iniA, SCALAR);
	void *solver = ((void *(*)(const dictionary *, Grid *, Grid *))solverAlloc)(iniA, rho, phi);
	void (*solveFn)(void *, Grid *, Grid *, const MpiInfo *) = (void (*)(void *, Grid *, Grid *, const MpiInfo *))solve;
	gCreateNeighborhood(iniA, mpiInfo, rho);
	gSetBndSlices(phi, mpiInfo);
	for (int s = 0; s < A->nSpecies; s++) printf("TWOPOP: qm A %d %.17g\n", s, A->charge[s] / A->mass[s]);
	for (int s = 0; s < B->nSpecies; s++) printf("TWOPOP: qm B %d %.17g\n", s, B->charge[s] / B->mass[s]);
	fflush(stdout);

	lattice_maxwell(iniA, A, mpiInfo, seedA, 0.25);
	extractEmigrants(A, mpiInfo);
	puMigrate(A, mpiInfo, rho);
	lattice_maxwell(iniB, B, mpiInfo, seedB, 0.);
	dump(A, dir, "A", "init");
	dump(B, dir, "B", "init");

	/* E of A's charge (main.c:168-176) */
	distr(A, rho);
	gHaloOp((funPtr)addSlice, rho, mpiInfo, FROMHALO);
	solveFn(solver, rho, phi, mpiInfo);
	gHaloOp((funPtr)setSlice, phi, mpiInfo, TOHALO);
	gFinDiff1st(phi, E);
	gHaloOp((funPtr)setSlice, E, mpiInfo, TOHALO);
	gMul(E, -1.);

	if (nine) {
		Population *more[8];
		acc(A, E);
		for (int k = 0; k < 8; k++) {
			more[k] = pAlloc(iniA);
			lattice_maxwell(iniA, more[k], mpiInfo, seedA + 1 + k, 0.);
			acc(more[k], E); /* (the ninth pending push ends the run here) */
		}
		msg(STATUS, "nine populations pushed without an error");
		for (int k = 0; k < 8; k++) pFree(more[k]);
	} else {
		if (!bonly) acc(A, E);
		if (!alone) acc(B, E);
		if (!strcmp(then, "drop")) extractEmigrants(A, mpiInfo);
		if (!strcmp(then, "move")) puMove(A, NULL);
		if (!strcmp(then, "free")) {
			pFree(A);
			A = NULL;
		}
		if (!strcmp(then, "ewrite") || !strcmp(then, "free")) gMul(E, 2.0);
		if (A && !bonly) dump(A, dir, "A", "end");
		if (!alone) dump(B, dir, "B", "end");
	}

	((void (*)(void *))solverFree)(solver);
	gFree(rho);
	gFree(phi);
	gFree(E);
	pFree(A);
	pFree(B);
	gFreeMpi(mpiInfo);
	uFree(unitsA);
	uFree(unitsB);
	free(scenario);
	free(thenKey);
	iniClose(iniA);
	iniClose(iniB);
	msg(STATUS, "PINC completed successfully!");
	return 0;
}
