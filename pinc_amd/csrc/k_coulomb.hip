// k_coulomb.hip -- binary Coulomb collisions between charged species
// (Takizuka & Abe 1977) for MI355X (gfx950): an extension, the reference has no
// collision module.  The rule is pinc_hip_coulomb's (include/pinc_hip.h).
//
//   k_cou_count    the cell of every particle (kept per particle), counts per cell
//   (scan)         pinc_hip_scan_keys over the cells
//   k_cou_scatter  the species-local indices, listed cell by cell (any order)
//   k_cou_pair     one wave per cell: the cell's list is ordered by the rule's
//                  hash keys and the collisions run one lane per pair
//
// k_cou_pair orders a list of up to kCouCap members in LDS by rank (the rank of
// a member is the number of members before it; every lane reads the same LDS
// word in the inner loop, a broadcast).  A longer list is ranked from global
// memory instead, the hash keys formed again for every comparison, into the
// per-particle array that held the cells: slow, the same order.  A workgroup is
// four waves with a list region each; they share the workgroup's barriers
// between the phases (load, rank, collide), whose loops are per wave.
//
// No two lanes write the same particle: a like pair's two members, a triple's
// three and an unlike B-member with all its partners belong to one lane.
//
// All arithmetic is fp64, products and sums are not fused (-ffp-contract=off).
#include "common.h"
#include <cmath>

using namespace pinc;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / PINC_WAVE;
constexpr int kCouCap = 128;  // members of a cell's list ordered in LDS
constexpr long kScanBlock = 4096;  // pinc_hip_scan_keys' work: 2 ceil(n / 4096) + 1 ints

// (the counter RNG of pinc_hip_init_species and pinc_hip_collide, k_particles.hip)
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
	z += 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}
__device__ __forceinline__ double uni(unsigned long long seed, unsigned long long c) {
	unsigned long long x = mix64(seed ^ mix64(c));
	return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// true cells of the rank per dimension
struct CouGrid {
	int T[3];
};

__device__ __forceinline__ int cou_cell(const CouGrid &g, double x, double y, double z) {
	const double p[3] = {x, y, z};
	int c = 0;
#pragma unroll
	for (int d = 2; d >= 0; d--) {
		const int i = (int)p[d];
		c = c * g.T[d] + ((i < 1 ? 1 : (i > g.T[d] ? g.T[d] : i)) - 1);
	}
	return c;
}

__global__ __launch_bounds__(kThreads) void k_cou_count(const double *__restrict__ x0, const double *__restrict__ x1,
                                                        const double *__restrict__ x2, long n, CouGrid g,
                                                        int *__restrict__ cellOf, int *__restrict__ cnt) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
		const int c = cou_cell(g, x0[i], x1[i], x2[i]);
		cellOf[i] = c;
		atomicAdd(&cnt[c], 1);
	}
}

// cur: zeroed; list[offs[c] + k] = the k-th particle to arrive at cell c
__global__ __launch_bounds__(kThreads) void k_cou_scatter(const int *__restrict__ cellOf, long n,
                                                          const int *__restrict__ offs, int *__restrict__ cur,
                                                          int *__restrict__ list) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
		const int c = cellOf[i];
		list[offs[c] + atomicAdd(&cur[c], 1)] = (int)i;
	}
}

// one species of a launch: its cell lists and its velocities (at its iStart)
struct CouSide {
	const int *offs;  // [nCells + 1]
	const int *list;  // [n] species-local indices, cell by cell
	int *ord;         // [n] the same in the rule's order, for lists above kCouCap
	double *v[3];
	unsigned long long keyOrd;   // the rule's key_s
	unsigned long long keyPair;  // the draws of the collisions whose first-named particle is of this species
	double frac;                 // mu / m of this species
};

struct CouArgs {
	CouSide s[2];
	int nCells;
	double K;
	double h[3];
	unsigned long long *counts;
};

__device__ __forceinline__ bool cou_before(unsigned long long ha, int ja, unsigned long long hb, int jb) {
	return ha < hb || (ha == hb && ja < jb);
}

__device__ __forceinline__ void cou_load(const CouSide &s, const double *h, int j, double *w) {
#pragma unroll
	for (int d = 0; d < 3; d++) w[d] = h[d] * s.v[d][j];
}
__device__ __forceinline__ void cou_store(const CouSide &s, const double *h, int j, const double *w) {
#pragma unroll
	for (int d = 0; d < 3; d++) s.v[d][j] = w[d] / h[d];
}

// One collision of p with q (the rule's "One collision"): kv = K nLow f, fp and
// fq the mass fractions, the draws u_k = uni(key, 4 j + k).  False if g == 0.
__device__ __forceinline__ bool cou_collide(double *wp, double *wq, double kv, double fp, double fq,
                                            unsigned long long key, unsigned long long j) {
	const double gx = wp[0] - wq[0], gy = wp[1] - wq[1], gz = wp[2] - wq[2];
	const double gp2 = gx * gx + gy * gy;
	const double gp = sqrt(gp2);
	const double g = sqrt(gp2 + gz * gz);
	if (!(g > 0.0)) return false;
	const double var = kv / ((g * g) * g);
	const double u0 = uni(key, 4ull * j);
	double sinT, omc;
	if (var < 1.0) {
		const double dl = (sqrt(var) * sqrt(-2.0 * log(u0))) * cospi(2.0 * uni(key, 4ull * j + 1));
		const double d2 = dl * dl, den = 1.0 + d2;
		sinT = (2.0 * dl) / den;
		omc = (2.0 * d2) / den;
	} else {
		const double c = 1.0 - 2.0 * u0;
		sinT = sqrt((1.0 - c) * (1.0 + c));
		omc = 1.0 - c;
	}
	double sp, cp;
	sincospi(2.0 * uni(key, 4ull * j + 2), &sp, &cp);
	const double sc = sinT * cp, ss = sinT * sp;
	double dx, dy, dz;
	if (gp > 0.0) {
		const double ex = gx / gp, ey = gy / gp;
		dx = ((ex * gz) * sc - (ey * g) * ss) - gx * omc;
		dy = ((ey * gz) * sc + (ex * g) * ss) - gy * omc;
		dz = -(gp * sc) - gz * omc;
	} else {
		dx = gz * sc;
		dy = gz * ss;
		dz = -(gz * omc);
	}
	wp[0] += fp * dx;
	wp[1] += fp * dy;
	wp[2] += fp * dz;
	wq[0] -= fq * dx;
	wq[1] -= fq * dy;
	wq[2] -= fq * dz;
	return true;
}

template <bool UNLIKE>
__global__ __launch_bounds__(kThreads) void k_cou_pair(CouArgs a) {
	constexpr int NS = UNLIKE ? 2 : 1;
	__shared__ CouArgs par;  // (as scalar arguments the parameters crowd the SGPRs: k_collide)
	__shared__ unsigned long long hash[kWaves][NS][kCouCap];
	__shared__ int idx[kWaves][NS][kCouCap];
	__shared__ int sorted[kWaves][NS][kCouCap];
	if (threadIdx.x == 0) par = a;
	__syncthreads();
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	unsigned long long done = 0;
	// the loop and its barriers are uniform over the workgroup
	for (long base = (long)blockIdx.x * kWaves; base < par.nCells; base += (long)gridDim.x * kWaves) {
		const long c = base + wv;
		const bool live = c < par.nCells;
		int o[NS], n[NS];
#pragma unroll
		for (int q = 0; q < NS; q++) {
			o[q] = live ? par.s[q].offs[c] : 0;
			n[q] = live ? par.s[q].offs[c + 1] - o[q] : 0;
		}
		// nothing to do in this cell: a like list below 2, an unlike pair with an empty side
		const bool idle = UNLIKE ? (n[0] == 0 || n[NS - 1] == 0) : n[0] < 2;
		// 1. the lists and their hash keys
		if (!idle) {
#pragma unroll
			for (int q = 0; q < NS; q++) {
				if (n[q] > kCouCap) continue;
				for (int t = lane; t < n[q]; t += 64) {
					const int j = par.s[q].list[o[q] + t];
					idx[wv][q][t] = j;
					hash[wv][q][t] = mix64(par.s[q].keyOrd ^ mix64((unsigned long long)j));
				}
			}
		}
		__syncthreads();
		// 2. rank every member
		if (!idle) {
#pragma unroll
			for (int q = 0; q < NS; q++) {
				if (n[q] <= kCouCap) {
					for (int t = lane; t < n[q]; t += 64) {
						const int j = idx[wv][q][t];
						const unsigned long long hj = hash[wv][q][t];
						int r = 0;
						for (int u = 0; u < n[q]; u++) r += cou_before(hash[wv][q][u], idx[wv][q][u], hj, j) ? 1 : 0;
						sorted[wv][q][r] = j;
					}
				} else {
					const int *l = par.s[q].list + o[q];
					const unsigned long long k = par.s[q].keyOrd;
					for (int t = lane; t < n[q]; t += 64) {
						const int j = l[t];
						const unsigned long long hj = mix64(k ^ mix64((unsigned long long)j));
						int r = 0;
						for (int u = 0; u < n[q]; u++) {
							const int ju = l[u];
							r += cou_before(mix64(k ^ mix64((unsigned long long)ju)), ju, hj, j) ? 1 : 0;
						}
						par.s[q].ord[o[q] + r] = j;
					}
				}
			}
		}
		__syncthreads();
		// 3. the collisions, one lane per pair
		if (!idle) {
			const int *S[NS];
#pragma unroll
			for (int q = 0; q < NS; q++) S[q] = n[q] <= kCouCap ? sorted[wv][q] : par.s[q].ord + o[q];
			if (!UNLIKE) {
				const CouSide &s = par.s[0];
				const int N = n[0];
				const double kv = par.K * (double)N;
				for (int t = lane; t < N / 2; t += 64) {
					if ((N & 1) && t == 0) {
						// the triple: (L0, L1), (L1, L2), (L2, L0), each with half the variance
						const int j0 = S[0][0], j1 = S[0][1], j2 = S[0][2];
						double w0[3], w1[3], w2[3];
						cou_load(s, par.h, j0, w0);
						cou_load(s, par.h, j1, w1);
						cou_load(s, par.h, j2, w2);
						const bool c01 = cou_collide(w0, w1, kv * 0.5, s.frac, s.frac, s.keyPair, j0);
						const bool c12 = cou_collide(w1, w2, kv * 0.5, s.frac, s.frac, s.keyPair, j1);
						const bool c20 = cou_collide(w2, w0, kv * 0.5, s.frac, s.frac, s.keyPair, j2);
						if (c01 || c20) cou_store(s, par.h, j0, w0);
						if (c01 || c12) cou_store(s, par.h, j1, w1);
						if (c12 || c20) cou_store(s, par.h, j2, w2);
						done += (c01 ? 1 : 0) + (c12 ? 1 : 0) + (c20 ? 1 : 0);
					} else {
						const int jp = S[0][2 * t + (N & 1)], jq = S[0][2 * t + (N & 1) + 1];
						double wp[3], wq[3];
						cou_load(s, par.h, jp, wp);
						cou_load(s, par.h, jq, wq);
						if (cou_collide(wp, wq, kv, s.frac, s.frac, s.keyPair, jp)) {
							cou_store(s, par.h, jp, wp);
							cou_store(s, par.h, jq, wq);
							done++;
						}
					}
				}
			} else {
				// A the longer list (species a on equal lengths), B the shorter
				const int ia = n[NS - 1] > n[0] ? NS - 1 : 0, ib = (NS - 1) - ia;
				const CouSide &sa = par.s[ia], &sb = par.s[ib];
				const int nA = n[ia], nB = n[ib];
				const int Q = nA / nB, R = nA - Q * nB;
				const double kv = par.K * (double)nB;
				for (int k = lane; k < nB; k += 64) {
					const int first = k < R ? k * (Q + 1) : R * (Q + 1) + (k - R) * Q;
					const int cnt = k < R ? Q + 1 : Q;
					const int jq = S[ib][k];
					double wq[3];
					cou_load(sb, par.h, jq, wq);
					bool any = false;
					for (int m = 0; m < cnt; m++) {
						const int jp = S[ia][first + m];
						double wp[3];
						cou_load(sa, par.h, jp, wp);
						if (cou_collide(wp, wq, kv, sa.frac, sb.frac, sa.keyPair, jp)) {
							cou_store(sa, par.h, jp, wp);
							any = true;
							done++;
						}
					}
					if (any) cou_store(sb, par.h, jq, wq);
				}
			}
		}
		__syncthreads();  // the lists are written again in the next round
	}
	done = wave_sum(done);
	if (lane == 0 && done) atomicAdd(par.counts, done);
}

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

}  // namespace

extern "C" long pinc_hip_coulomb_cell_cap(void) { return kCouCap; }

// per species: counts, then cursors [nCells + 1] | offsets [nCells + 1] | the
// particles' cells, then the ordered long lists [n] | the lists [n]; and
// pinc_hip_scan_keys' work once
extern "C" long pinc_hip_coulomb_work(long nA, long nB, long nCells) {
	if (nA < 0 || nB < 0 || nCells < 0) return -1;
	return 4 * (nCells + 1) + 2 * (nA + nB) + 2 * ceil_div(nCells, kScanBlock) + 1;
}

extern "C" unsigned long long pinc_hip_coulomb_key(unsigned long long seed, unsigned long long step, int rank, int a,
                                                   int b) {
	const unsigned long long pair = (unsigned long long)(a * PINC_MAX_SPECIES + b);
	return mix64(pinc_hip_collide_key(seed, step, rank, a) ^ 0x636F756C6F6D62ULL ^ mix64(pair));
}

extern "C" int pinc_hip_coulomb(pinc_pop_t pop, int a, int b, pinc_geom_t g, pinc_coulomb_t c, int *work, long workInts,
                                unsigned long long *counts, void *stream) {
	if (a < 0 || b >= pop.nSpecies || a > b) return set_error(hipErrorInvalidValue, "coulomb: bad species pair");
	if (pop.nd != 3 || g.nd != 3) return set_error(hipErrorInvalidValue, "coulomb: three dimensions only");
	if (!work || !counts) return set_error(hipErrorInvalidValue, "coulomb: null scratch or counter");
	for (int d = 0; d < 3; d++) {
		if (!pop.x[d] || !pop.v[d]) return set_error(hipErrorInvalidValue, "coulomb: null particle array");
		if (!(c.h[d] > 0.0) || !std::isfinite(c.h[d])) return set_error(hipErrorInvalidValue, "coulomb: h must be > 0");
	}
	if (!(c.K >= 0.0) || !std::isfinite(c.K)) return set_error(hipErrorInvalidValue, "coulomb: K negative or not finite");
	if (!(c.fa > 0.0 && c.fa < 1.0 && c.fb > 0.0 && c.fb < 1.0))
		return set_error(hipErrorInvalidValue, "coulomb: a mass fraction outside (0, 1)");
	const CouGrid cg = {{g.T[0], g.T[1], g.nloc}};
	if (cg.T[0] < 1 || cg.T[1] < 1 || cg.T[2] < 1) return set_error(hipErrorInvalidValue, "coulomb: an empty grid");
	const long nCells = (long)cg.T[0] * cg.T[1] * cg.T[2];
	const int ns = a == b ? 1 : 2;
	const int sp[2] = {a, b};
	Span span[2];
	for (int q = 0; q < 2; q++) {
		span[q] = species_span(pop, sp[q]);
		if (span[q].n < 0 || pop.iStop[sp[q]] > pop.iStart[sp[q] + 1])
			return set_error(hipErrorInvalidValue, "coulomb: a species' live range is outside its slots");
	}
	if (nCells >= (1L << 31) - 1 || span[0].n >= (1L << 31) || span[1].n >= (1L << 31))
		return set_error(hipErrorInvalidValue, "coulomb: too many cells or particles");
	if (workInts < pinc_hip_coulomb_work(span[0].n, ns == 2 ? span[1].n : 0, nCells))
		return set_error(hipErrorInvalidValue, "coulomb: work too small");
	// nothing to pair: K = 0 switches the pair off
	if (c.K == 0.0 || span[0].n == 0 || span[1].n == 0 || (ns == 1 && span[0].n < 2)) return 0;

	hipStream_t st = (hipStream_t)stream;
	CouArgs args;
	args.nCells = (int)nCells;
	args.K = c.K;
	for (int d = 0; d < 3; d++) args.h[d] = c.h[d];
	args.counts = counts;
	int *w = work;
	int *scanWork = work + 4 * (nCells + 1) + 2 * (span[0].n + (ns == 2 ? span[1].n : 0));
	for (int q = 0; q < ns; q++) {
		const long n = span[q].n;
		int *cnt = w, *offs = w + (nCells + 1), *cellOf = offs + (nCells + 1), *list = cellOf + n;
		w = list + n;
		hipError_t e = hipMemsetAsync(cnt, 0, (nCells + 1) * sizeof(int), st);
		if (e != hipSuccess) return set_error(e, "coulomb: memset");
		long nb = ceil_div(n, (long)kThreads);
		if (nb > 65536L * 8) nb = 65536L * 8;
		const auto x = upto_nd(pop.x, 3, span[q].b0);
		hipLaunchKernelGGL(k_cou_count, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, n, cg, cellOf, cnt);
		if (int rc = pinc_hip_scan_keys(cnt, nCells, offs, scanWork, stream)) return rc;
		e = hipMemsetAsync(cnt, 0, (nCells + 1) * sizeof(int), st);
		if (e != hipSuccess) return set_error(e, "coulomb: memset");
		hipLaunchKernelGGL(k_cou_scatter, dim3(nb), dim3(kThreads), 0, st, cellOf, n, offs, cnt, list);
		CouSide &s = args.s[q];
		s.offs = offs;
		s.list = list;
		s.ord = cellOf;  // (the cells are not read again)
		for (int d = 0; d < 3; d++) s.v[d] = pop.v[d] + span[q].b0;
		s.keyOrd = mix64(c.key ^ (unsigned long long)(1 + q));
		s.keyPair = mix64(c.key ^ (unsigned long long)(3 + q));
		s.frac = q == 0 ? c.fa : c.fb;
	}
	if (ns == 1) args.s[1] = args.s[0];
	long nb = ceil_div(nCells, (long)kWaves);
	if (nb > 65536L * 8) nb = 65536L * 8;
	if (ns == 1)
		hipLaunchKernelGGL(k_cou_pair<false>, dim3(nb), dim3(kThreads), 0, st, args);
	else
		hipLaunchKernelGGL(k_cou_pair<true>, dim3(nb), dim3(kThreads), 0, st, args);
	return check_launch("coulomb");
}
