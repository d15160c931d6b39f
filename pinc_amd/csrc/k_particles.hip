// k_particles.hip -- particle kernels of the PINC hot path for MI355X (gfx950).
//
//   move + classify     puMove (pusher.c:86-119) fused with the neighbour test
//                       of puExtractEmigrants3D/ND (pusher.c:782-910)
//   extract             the reference's serial back-fill compaction, made
//                       parallel without changing its result or the order in
//                       which emigrants are listed (DESIGN.md "Migration")
//   import              shiftImmigrants + importParticles (pusher.c:941-985)
//   deposit             puDistr3D1 / puDistrND1 (pusher.c:512-638)
//   moments             per-species velocity moments with the deposit's
//                       weights (an extension, not in the reference)
//   phase space         per-species histograms over one or two coordinates
//                       (an extension, not in the reference)
//   accelerate         puAcc3D1KE / puAccND1KE + interpolators
//                       (pusher.c:178-265, 1089-1162)
//   init                pPosLattice / pPosPerturb / pVel* (population.c)
//
// All arithmetic is fp64 in the reference's association order; the library
// is compiled with -ffp-contract=off so no multiply-add is fused.
#include "common.h"
#include <type_traits>

using namespace pinc;

namespace {

struct Thr {
	double lo[3], up[3], hi[3];
	int T[3];  // true cells per dimension (local)
};

constexpr int kThreads = 256;
constexpr int kItems = PINC_CHUNK / kThreads;

__device__ __forceinline__ unsigned long long lanemask_lt() {
	return (1ull << (threadIdx.x & 63)) - 1ull;
}

// ------------------------------------------------------------ move --------
template <int ND>
__global__ __launch_bounds__(kThreads) void k_move_classify(
		double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ x2,
		const double *__restrict__ v0, const double *__restrict__ v1,
		const double *__restrict__ v2, long n, int doMove, Thr thr, int center,
		unsigned char *__restrict__ flags, int *__restrict__ chunkCount, double maxVel,
		int *__restrict__ err, int wrapMask) {
	__shared__ int wcnt[kThreads / 64];
	double *xs[3] = {x0, x1, x2};
	const double *vs[3] = {v0, v1, v2};
	long base = (long)blockIdx.x * PINC_CHUNK;
	int cnt = 0;
	int bad = 0;
#pragma unroll 2
	for (int k = 0; k < kItems; k++) {
		long i = base + k * kThreads + threadIdx.x;
		if (i >= n) break;
		double p[ND];
#pragma unroll
		for (int d = 0; d < ND; d++) {
			p[d] = xs[d][i];
			if (doMove) {
				double v = vs[d][i];
				bad |= (v > maxVel);  // pVelAssertMax (population.c:342-365)
				p[d] += v;
				xs[d][i] = p[d];
			}
		}
		int ne = 0;
#pragma unroll
		for (int d = ND - 1; d >= 0; d--) {
			int dig = 1 - (p[d] < thr.lo[d]) + (p[d] >= thr.up[d]);
			// pPosAssertInLocalFrame after the periodic shift (population.c:316-340)
			double q = p[d] - (double)(dig - 1) * (thr.hi[d] - 1.0);
			bad |= (q < 0.0 || q > thr.hi[d]) << 1;
			if ((wrapMask >> d) & 1) {
				// tiled layout: a crossing of a rank-local periodic boundary is
				// applied in place with the import's shift (pusher.c:941-964)
				if (dig != 1) {
					p[d] = p[d] + (double)((1 - dig) * thr.T[d]);
					xs[d][i] = p[d];
				}
				dig = 1;
			}
			ne = ne * 3 + dig;
		}
		flags[i] = (unsigned char)ne;
		cnt += (ne != center);
	}
	if (bad) atomicOr(err, bad);
	int wsum = wave_sum(cnt);
	if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = wsum;
	__syncthreads();
	if (threadIdx.x == 0) {
		int t = 0;
		for (int w = 0; w < kThreads / 64; w++) t += wcnt[w];
		chunkCount[blockIdx.x] = t;
	}
}

// --------------------------------------------------- single-block scans ---
// exclusive scan of in[0..n) into out[0..n], out[n] = total
__global__ __launch_bounds__(1024) void k_scan_single(const int *__restrict__ in,
                                                      int *__restrict__ out, int n) {
	__shared__ long part[1024];
	int t = threadIdx.x;
	int seg = (n + 1023) / 1024;
	int a = t * seg, b = min(n, a + seg);
	long s = 0;
	for (int i = a; i < b; i++) s += in[i];
	part[t] = s;
	__syncthreads();
	for (int o = 1; o < 1024; o <<= 1) {
		long v = (t >= o) ? part[t - o] : 0;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	long run = part[t] - s;
	for (int i = a; i < b; i++) {
		int v = in[i];
		out[i] = (int)run;
		run += v;
	}
	if (t == 1023) out[n] = (int)part[1023];
}

// ----------------------------------------------------------- extract ------
// Per particle j (relative to the species start) with E(j) = emigrants
// before j, n particles, E emigrants, m = n-E survivors:
//   emigrant j<m   is hole number k=E(j)+1
//   survivor j>=m  is tail survivor number r = n-j-E+E(j) (counted from the end)
//   emigrant j>m   is extracted at position n-j
// (derivation: DESIGN.md "Migration"; checked against the serial loop).
__global__ __launch_bounds__(kThreads) void k_extract_a(
		const unsigned char *__restrict__ flags, long n, int center,
		const int *__restrict__ chunkOffset, int nChunks, int *__restrict__ tail,
		int *__restrict__ holes, int *__restrict__ order, int *__restrict__ scratch) {
	__shared__ int wtot[kThreads / 64];
	long E = chunkOffset[nChunks];
	long m = n - E;
	long base = (long)blockIdx.x * PINC_CHUNK;
	int running = chunkOffset[blockIdx.x];
	// a chunk with no emigrants wholly before m has no holes and no tail
	// survivors: nothing to record (most chunks when few particles leave)
	if (chunkOffset[blockIdx.x + 1] == running && base + PINC_CHUNK <= m) return;
	int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	for (int k = 0; k < kItems; k++) {
		long i = base + k * kThreads + threadIdx.x;
		bool in = i < n;
		bool emig = in && flags[i] != center;
		unsigned long long b = __ballot(emig);
		int rw = __popcll(b & lanemask_lt());
		if (lane == 0) wtot[w] = __popcll(b);
		__syncthreads();
		int before = 0, tot = 0;
		for (int q = 0; q < kThreads / 64; q++) {
			before += (q < w) ? wtot[q] : 0;
			tot += wtot[q];
		}
		long Ej = running + before + rw;
		if (in) {
			if (emig) {
				if (i < m) holes[Ej + 1] = (int)i;
				else if (i > m) order[n - i] = (int)i;
			} else if (i >= m) {
				tail[n - i - E + Ej] = (int)i;
			}
			if (i == m) scratch[0] = (int)Ej;  // number of holes
		}
		running += tot;
		__syncthreads();
	}
}

__global__ void k_extract_b(const unsigned char *__restrict__ flags, long n, long E, int center,
                            const int *__restrict__ tail, const int *__restrict__ holes,
                            int *__restrict__ order, const int *__restrict__ scratch) {
	long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
	long m = n - E;
	int h = scratch[0];
	if (q >= 1 && q <= h) {
		long prevT = (q == 1) ? n : tail[q - 1];
		order[n - prevT] = holes[q];
	}
	if (q == 0 && m < n && flags[m] != center) {
		long t = h ? tail[h] : n;
		order[n - t] = (int)m;
	}
}

// per-block direction histogram over the extraction order
constexpr int kRankItems = 4;
constexpr int kRankChunk = kThreads * kRankItems;
constexpr int kMaxNe = PINC_NE_CODES;  // 27 directions + the object sink

__global__ __launch_bounds__(kThreads) void k_rank_hist(const unsigned char *__restrict__ flags,
                                                        const int *__restrict__ order, long E,
                                                        int *__restrict__ blockHist) {
	__shared__ int hist[kMaxNe];
	if (threadIdx.x < kMaxNe) hist[threadIdx.x] = 0;
	__syncthreads();
	long base = (long)blockIdx.x * kRankChunk;
	for (int k = 0; k < kRankItems; k++) {
		long p = base + k * kThreads + threadIdx.x;
		if (p < E) atomicAdd(&hist[flags[order[p]]], 1);
	}
	__syncthreads();
	if (threadIdx.x < kMaxNe) blockHist[(long)blockIdx.x * kMaxNe + threadIdx.x] = hist[threadIdx.x];
}

// exclusive scan per direction over blocks; bases per direction; counts
__global__ __launch_bounds__(kMaxNe * 32) void k_hist_scan(int *__restrict__ blockHist, int nb,
                                                           int *__restrict__ scratch) {
	// scratch[32..32+kMaxNe): base of each direction, scratch[64..64+kMaxNe): count
	__shared__ int tot[kMaxNe];
	int ne = threadIdx.x >> 5, l = threadIdx.x & 31;
	if (ne < kMaxNe && l == 0) {
		int run = 0;
		for (int b = 0; b < nb; b++) {
			int v = blockHist[(long)b * kMaxNe + ne];
			blockHist[(long)b * kMaxNe + ne] = run;
			run += v;
		}
		tot[ne] = run;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		int run = 0;
		for (int q = 0; q < kMaxNe; q++) {
			scratch[32 + q] = run;
			scratch[64 + q] = tot[q];
			run += tot[q];
		}
	}
}

// stable scatter of emigrants into the direction-ordered buffer
__global__ __launch_bounds__(kThreads) void k_rank_scatter(
		unsigned char *__restrict__ flags, const int *__restrict__ order, long E,
		const int *__restrict__ blockHist, const int *__restrict__ scratch, pinc_pop_t pop,
		long sbase, double *__restrict__ buf, long cap, unsigned char *__restrict__ bufNe, int center) {
	__shared__ int waveCnt[kThreads / 64][kMaxNe];
	__shared__ int running[kMaxNe];
	int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (threadIdx.x < kMaxNe) running[threadIdx.x] = 0;
	long base = (long)blockIdx.x * kRankChunk;
	for (int k = 0; k < kRankItems; k++) {
		for (int q = threadIdx.x; q < (kThreads / 64) * kMaxNe; q += kThreads)
			(&waveCnt[0][0])[q] = 0;
		__syncthreads();
		long p = base + k * kThreads + threadIdx.x;
		bool in = p < E;
		int j = in ? order[p] : 0;
		int ne = in ? flags[j] : 31;
		// lanes with the same direction (match-any over 5 bits)
		unsigned long long same = __ballot(in);
#pragma unroll
		for (int bit = 0; bit < 5; bit++) {
			unsigned long long bb = __ballot((ne >> bit) & 1);
			same &= ((ne >> bit) & 1) ? bb : ~bb;
		}
		int rw = __popcll(same & lanemask_lt());
		if (in && rw == 0) waveCnt[w][ne] = __popcll(same);
		__syncthreads();
		if (in) {
			int off = running[ne] + rw;
			for (int q = 0; q < w; q++) off += waveCnt[q][ne];
			long dst = (long)scratch[32 + ne] + blockHist[(long)blockIdx.x * kMaxNe + ne] + off;
			long src = sbase + j;
			for (int d = 0; d < pop.nd; d++) {
				buf[d * cap + dst] = pop.x[d][src];
				buf[(3 + d) * cap + dst] = pop.v[d][src];
			}
			bufNe[dst] = (unsigned char)ne;
			flags[j] = (unsigned char)center;  // (read above by this thread only: the species' flags are
			                                   // all the centre again after the extraction)
		}
		__syncthreads();
		if (threadIdx.x < kMaxNe) {
			int t = 0;
			for (int q = 0; q < kThreads / 64; q++) t += waveCnt[q][threadIdx.x];
			running[threadIdx.x] += t;
		}
		__syncthreads();
	}
}

__global__ void k_fill_holes(pinc_pop_t pop, long sbase, const int *__restrict__ tail,
                             const int *__restrict__ holes, const int *__restrict__ scratch) {
	long k = (long)blockIdx.x * blockDim.x + threadIdx.x + 1;
	int h = scratch[0];
	if (k > h) return;
	long src = sbase + tail[k], dst = sbase + holes[k];
	for (int d = 0; d < pop.nd; d++) {
		pop.x[d][dst] = pop.x[d][src];
		pop.v[d][dst] = pop.v[d][src];
	}
}

__global__ void k_import(pinc_pop_t pop, long dst, const double *__restrict__ buf, long cap,
                         const unsigned char *__restrict__ bufNe, long first, long n, int T0,
                         int T1, int T2, int shiftMask) {
	long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n) return;
	long e = first + q;
	int ne = bufNe[e];
	int T[3] = {T0, T1, T2};
	for (int d = 0; d < pop.nd; d++) {
		int dig = ne % 3;
		ne /= 3;
		// receiver tag t = reciprocal(ne): shift = (digit_d(t)-1)*T_d = (1-dig)*T_d
		double shift = ((shiftMask >> d) & 1) ? (double)((1 - dig) * T[d]) : 0.0;
		pop.x[d][dst + q] = buf[d * cap + e] + shift;
		pop.v[d][dst + q] = buf[(3 + d) * cap + e];
	}
}

__global__ void k_pack(const double *__restrict__ buf, long cap, const unsigned char *__restrict__ bufNe,
                       long first, long n, int nd, double *__restrict__ out) {
	long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n) return;
	long e = first + q;
	double *r = out + q * PINC_REC;
	for (int d = 0; d < 3; d++) {
		r[d] = d < nd ? buf[d * cap + e] : 0.0;
		r[3 + d] = d < nd ? buf[(3 + d) * cap + e] : 0.0;
	}
	r[6] = (double)bufNe[e];
}

__global__ void k_import_rec(pinc_pop_t pop, long dst, const double *__restrict__ rec, long n, int T0,
                             int T1, int T2) {
	long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n) return;
	const double *r = rec + q * PINC_REC;
	int ne = (int)r[6];
	int T[3] = {T0, T1, T2};
	for (int d = 0; d < pop.nd; d++) {
		int dig = ne % 3;
		ne /= 3;
		pop.x[d][dst + q] = r[d] + (double)((1 - dig) * T[d]);
		pop.v[d][dst + q] = r[3 + d];
	}
}

// ---------------------------------------------------------- deposit -------
struct Geo {
	int T[3];      // storage extent per dim (slab dim: nloc)
	long stride[3];
	int slab;      // slab dimension
};

__device__ __forceinline__ Geo make_geo(const pinc_geom_t &g) {
	// fully unrolled: no dynamically indexed register arrays (scratch)
	Geo r;
	r.slab = g.nd - 1;
	long s = 1;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		r.T[d] = (d == r.slab) ? g.nloc : g.T[d];
		r.stride[d] = s;
		if (d < g.nd) s *= (d == r.slab) ? (long)(g.nloc + 2) : (long)r.T[d];
	}
	return r;
}

// storage coordinate of padded node coordinate p in dim d
__device__ __forceinline__ long node_off(const Geo &G, int d, int p) {
	int s = (d == G.slab) ? p : wrap_pad(p, G.T[d]);
	return (long)s * G.stride[d];
}

// --------------------------------------------- LDS-privatised deposit -----
// The frame shared by the kernels that scatter a species through an LDS box
// owned by the workgroup (k_deposit_tiled, k_moments, k_phase_hist,
// k_deposit_tsc; the box also k_deposit_cells), each piece written once below:
//  * ChunkItems: a workgroup owns a chunk of kThreads * ITEMS consecutive
//    particles, a thread ITEMS consecutive ones, loaded 16 B at a time from
//    the 16-byte aligned slot at or below iStart; the guards of an odd iStart
//    and of the partial last chunk are load2() and live();
//  * BlockBounds: the block's minimum, maximum (and sum) of per-thread integer
//    bounds, and one more count, through DPP wave reductions and LDS.  Which
//    box follows from them is each kernel's policy;
//  * NodeBox: a box of grid nodes in LDS: zero(), the index of a cell whose
//    upper neighbours are inside too (of a node whose lower and upper
//    neighbours are: the order-2 stencil), the corners' offsets, and the flush with
//    one global atomic per value that is not zero;
//  * cell_split: a particle's cell, the fractions of its CIC weights, and
//    whether it continues the thread's run of particles in one cell.
//
// k_deposit_tiled: in either layout (the reference's order, spatially
// coherent from the lattice start, or the cell-sorted tiled layout)
// consecutive particles mostly share a cell and a chunk covers a small box of
// nodes:
//  * a thread sums the eight weights of a run of particles in one cell in
//    registers and adds them once (cell-sorted: once per kDepItems);
//  * the chunk's bounding box is accumulated in LDS (ds_add_f64) and flushed.
// Chunks whose box exceeds the LDS tile use the same run accumulation with
// global atomics.  Weights are the reference's expressions (pusher.c:550-565,
// 626-638); only the summation order differs from the serial loop.
constexpr int kDepItems = 16;
constexpr int kDepChunk = kThreads * kDepItems;
constexpr int kDepCap = 4096;  // LDS nodes per workgroup (32 KiB)

// Integer wave reductions with DPP (row shifts 1, 2, 4, 8, then the row
// broadcasts of lanes 15 and 31): six VALU instructions with DPP operands and
// one readlane, the total uniform.  (The shfl_xor butterflies they replace
// cost six ds_bpermute round trips through the LDS unit each: in the push,
// where nine reductions per block ran that way, a third of its LDS
// instructions.)  Every lane of the wave must be active.
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i(int old, int v) {
	return __builtin_amdgcn_update_dpp(old, v, CTRL, ROWS, 0xf, false);
}
template <typename Op>
__device__ __forceinline__ int wave_reduce_i(int v, int id, Op op) {
	v = op(v, dpp_i<0x111, 0xf>(id, v));  // row_shr:1
	v = op(v, dpp_i<0x112, 0xf>(id, v));  // row_shr:2
	v = op(v, dpp_i<0x114, 0xf>(id, v));  // row_shr:4
	v = op(v, dpp_i<0x118, 0xf>(id, v));  // row_shr:8 (lane 15 of a row: its total)
	v = op(v, dpp_i<0x142, 0xa>(id, v));  // row_bcast:15 into rows 1, 3
	v = op(v, dpp_i<0x143, 0xc>(id, v));  // row_bcast:31 into rows 2, 3
	return __builtin_amdgcn_readlane(v, 63);
}
// fp64 wave sum, the same DPP pattern on the two halves of each partner
// value (a fixed tree: deterministic); the total in every lane's return
__device__ __forceinline__ double wave_sum_d(double v) {
	auto step = [](double x, auto ctrl) -> double {
		constexpr int C = decltype(ctrl)::value >> 4, R = decltype(ctrl)::value & 15;
		const unsigned long long u = __double_as_longlong(x);
		const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)u, C, R, 0xf, false);
		const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(u >> 32), C, R, 0xf, false);
		return x + __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
	};
	v = step(v, std::integral_constant<int, (0x111 << 4) | 0xf>{});
	v = step(v, std::integral_constant<int, (0x112 << 4) | 0xf>{});
	v = step(v, std::integral_constant<int, (0x114 << 4) | 0xf>{});
	v = step(v, std::integral_constant<int, (0x118 << 4) | 0xf>{});
	v = step(v, std::integral_constant<int, (0x142 << 4) | 0xa>{});
	v = step(v, std::integral_constant<int, (0x143 << 4) | 0xc>{});
	const unsigned long long u = __double_as_longlong(v);
	const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, 63), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), 63);
	return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int wave_min_i(int v) {
	return wave_reduce_i(v, INT32_MAX, [](int a, int b) { return min(a, b); });
}
__device__ __forceinline__ int wave_max_i(int v) {
	return wave_reduce_i(v, INT32_MIN, [](int a, int b) { return max(a, b); });
}
__device__ __forceinline__ int wave_sum_i(int v) {
	return wave_reduce_i(v, 0, [](int a, int b) { return a + b; });
}

template <int ND, bool V3D>
__device__ __forceinline__ void cic_weights(const double *dec, const double *comp, double *w) {
	if (V3D) {
		double xc = comp[0], yc = comp[1], zc = comp[2];
		double x = dec[0], y = dec[1], z = dec[2];
		w[0] = xc * yc * zc;
		w[1] = x * yc * zc;
		w[2] = xc * y * zc;
		w[3] = x * y * zc;
		w[4] = xc * yc * z;
		w[5] = x * yc * z;
		w[6] = xc * y * z;
		w[7] = x * y * z;
	} else {
#pragma unroll
		for (int c = 0; c < (1 << ND); c++) {
			double f = 1.0;
#pragma unroll
			for (int d = ND - 1; d >= 1; d--) f = (((c >> d) & 1) ? dec[d] : comp[d]) * f;
			w[c] = ((c & 1) ? dec[0] : comp[0]) * f;
		}
	}
}

// main.c's literal loop adds rho's ghost layers twice (main.c:226,232): a
// weight that lands on a periodic ghost node counts 2^g times, g = its ghost
// coordinates (checked against grid.c:340-406 applied twice).  Slab ghost
// planes are kept on the device and folded twice by the caller; here the
// non-slab dimensions, which are wrapped at deposit, get their factor.
// literal == 2 is the second fold of a deposit made without that factor
// (main.c's loop calling gHaloOp(addSlice, rho, FROMHALO) twice on a library
// that was not told in advance, pinc_grid.c): the weight still missing,
// (2^g_xy - 1) w, and twice that on a slab ghost plane, which the second fold
// adds once more.
template <int ND>
__device__ __forceinline__ double literal_node_factor(const pinc_geom_t &g, const int *p) {
	const int slab = g.nd - 1;
	double m = 1.0, mz = 1.0;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		if (d == slab) {
			if (g.literal == 2 && (p[d] == 0 || p[d] == g.nloc + 1)) mz = 2.0;
			continue;
		}
		if (p[d] == 0 || p[d] == g.T[d] + 1) m *= 2.0;
	}
	return g.literal == 2 ? (m - 1.0) * mz : m;
}

template <int ND>
__device__ __forceinline__ void literal_ghost_weights(const pinc_geom_t &g, const int *j, double *w) {
	if (!g.literal) return;
#pragma unroll
	for (int c = 0; c < (1 << ND); c++) {
		int p[3];
#pragma unroll
		for (int d = 0; d < ND; d++) p[d] = j[d] + ((c >> d) & 1);
		w[c] *= literal_node_factor<ND>(g, p);
	}
}

// global offset of padded node (j[0]+c0, j[1]+c1, ...) for corner c
template <int ND>
__device__ __forceinline__ long corner_off(const Geo &G, const int *j, int c) {
	long off = 0;
#pragma unroll
	for (int d = 0; d < ND; d++) off += node_off(G, d, j[d] + ((c >> d) & 1));
	return off;
}

constexpr int kWaves = kThreads / 64;

// A thread's ITEMS consecutive particles of its workgroup's chunk: slots i0 ..
// i0 + ITEMS - 1 of the species [b0, end), i0 even relative to the 16-byte
// aligned slot at or below b0.
template <int ITEMS>
struct ChunkItems {
	long i0, b0, end;
	unsigned valid;  // bit k: slot i0 + k is a particle of the species
	__device__ __forceinline__ ChunkItems(long first, long n) : b0(first), end(first + n) {
		i0 = (b0 & ~1L) + (long)blockIdx.x * (kThreads * ITEMS) + (long)threadIdx.x * ITEMS;
		valid = 0;
#pragma unroll
		for (int k = 0; k < ITEMS; k++) valid |= (unsigned)(i0 + k >= b0 && i0 + k < end) << k;
	}
	__device__ __forceinline__ bool live(int k) const { return (valid >> k) & 1u; }
	// p[i0 + k], p[i0 + k + 1] (k even): one 16-byte load where both are live,
	// else each on its own, 0 for a slot that is not
	__device__ __forceinline__ void load2(const double *p, int k, double &a, double &b) const {
		long i = i0 + k;
		if (i >= b0 && i + 1 < end) {
			double2 v = *reinterpret_cast<const double2 *>(p + i);
			a = v.x;
			b = v.y;
		} else {
			a = (i >= b0 && i < end) ? p[i] : 0.0;
			b = (i + 1 >= b0 && i + 1 < end) ? p[i + 1] : 0.0;
		}
	}
};
// workgroups of a species [b0, b0 + n) in chunks of `chunk` particles
inline long chunk_blocks(long b0, long n, long chunk) { return (n + (b0 & 1L) + chunk - 1) / chunk; }

// cell of a coordinate; CLAMP keeps it inside the slab (0..T)
template <bool CLAMP>
__device__ __forceinline__ int cell_of(double x, int T) {
	return CLAMP ? min(max((int)x, 0), T) : (int)x;
}

// A particle's cell j, its fractions dec and comp = 1 - dec of the CIC
// weights, and whether j is the cell cj of the thread's current run.
template <int ND, bool CLAMP>
__device__ __forceinline__ bool cell_split(const double *x, const int *T, const int *cj, int *j, double *dec,
                                           double *comp) {
	bool same = true;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		j[d] = cell_of<CLAMP>(x[d], T[d]);
		dec[d] = x[d] - j[d];
		comp[d] = 1 - dec[d];
		same = same && (j[d] == cj[d]);
	}
	return same;
}

// lo, hi (the upper node, cell + 1) and sum of the cells of a thread's live
// particles along one dimension (p: that coordinate's array)
template <bool CLAMP, int ITEMS>
__device__ __forceinline__ void chunk_cell_bounds(const ChunkItems<ITEMS> &ch, const double *p, int T, int &lo,
                                                  int &hi, int &sum) {
#pragma unroll
	for (int k = 0; k < ITEMS; k += 2) {
		double x[2];
		ch.load2(p, k, x[0], x[1]);
#pragma unroll
		for (int h = 0; h < 2; h++)
			if (ch.live(k + h)) {
				const int c = cell_of<CLAMP>(x[h], T);
				lo = min(lo, c);
				hi = max(hi, c + 1);
				sum += c;
			}
	}
}

// Block reduction of per-thread bounds (in LDS: __shared__): minimum of lo[d],
// maximum of hi[d] and, with SUM, the sum of sum[d] for d < nd <= N, and with
// EXTRA the sum of one more integer.  reduce() is called by every thread and
// ends in a barrier; after it any thread reads the block's values with get()
// and extra().
template <int N, bool SUM, bool EXTRA>
struct BlockBounds {
	static constexpr int S = SUM ? 3 : 2;
	int red[(S * N + (EXTRA ? 1 : 0)) * kWaves];
	__device__ __forceinline__ void reduce(int nd, const int *lo, const int *hi, const int *sum, int extra) {
		const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
		for (int d = 0; d < nd; d++) {
			const int a = wave_min_i(lo[d]), b = wave_max_i(hi[d]);
			int c = 0;
			if constexpr (SUM) c = wave_sum_i(sum[d]);
			if (lane == 0) {
				red[(S * d) * kWaves + wv] = a;
				red[(S * d + 1) * kWaves + wv] = b;
				if constexpr (SUM) red[(S * d + 2) * kWaves + wv] = c;
			}
		}
		if constexpr (EXTRA) {
			const int c = wave_sum_i(extra);
			if (lane == 0) red[S * N * kWaves + wv] = c;
		}
		__syncthreads();
	}
	__device__ __forceinline__ void get(int d, int &lo, int &hi, int &sum) const {
		lo = INT32_MAX, hi = INT32_MIN, sum = 0;
		for (int w = 0; w < kWaves; w++) {
			lo = min(lo, red[(S * d) * kWaves + w]);
			hi = max(hi, red[(S * d + 1) * kWaves + w]);
			if constexpr (SUM) sum += red[(S * d + 2) * kWaves + w];
		}
	}
	__device__ __forceinline__ int extra() const {
		static_assert(EXTRA, "no extra count in this layout");
		int c = 0;
		for (int w = 0; w < kWaves; w++) c += red[S * N * kWaves + w];
		return c;
	}
};

// A box of grid nodes lo[d] .. lo[d] + n[d] - 1 (padded node coordinates)
// that a workgroup accumulates in LDS, perNode values per node, value-major;
// vol = 0: no box.  Block-uniform.
template <int ND>
struct NodeBox {
	int lo[3] = {0, 0, 0}, n[3] = {1, 1, 1}, st[3] = {0, 0, 0};
	int vol = 0;
	NodeBox() = default;
	__device__ __forceinline__ NodeBox(const int *first, const int *extent) {
		vol = 1;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			lo[d] = first[d];
			n[d] = extent[d];
			st[d] = vol;
			vol *= n[d];
		}
	}
	__device__ __forceinline__ void zero(double *acc, int perNode) const {
		for (int t = threadIdx.x; t < vol * perNode; t += kThreads) acc[t] = 0.0;
	}
	// l0: the linear index of the lower node of `cell`; true if the cell's
	// upper neighbours are inside the box too
	__device__ __forceinline__ bool index(const int *cell, int &l0) const {
		bool in = true;
		l0 = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			const int r = cell[d] - lo[d];
			in = in && r >= 0 && r + 1 < n[d];
			l0 += r * st[d];
		}
		return in;
	}
	// l: the linear index of `node`; true if its lower and upper neighbours
	// are inside the box too (a three-node stencil per dimension)
	__device__ __forceinline__ bool index_centre(const int *node, int &l) const {
		bool in = true;
		l = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			const int r = node[d] - lo[d];
			in = in && r >= 1 && r + 1 < n[d];
			l += r * st[d];
		}
		return in;
	}
	// offset of corner c (bit d: the upper node along d) from a cell's index
	__device__ __forceinline__ int corner(int c) const {
		int off = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) off += ((c >> d) & 1) ? st[d] : 0;
		return off;
	}
	// after a barrier: one global atomic per value that is not zero, in
	// storage order
	__device__ __forceinline__ void flush(const double *acc, int perNode, const Geo &G, double *dst) const {
		for (int t = threadIdx.x; t < vol * perNode; t += kThreads) {
			const double v = acc[t];
			if (v == 0.0) continue;
			int r = t / perNode;
			const int m = t - r * perNode;
			long off = 0;
#pragma unroll
			for (int d = 0; d < ND; d++) {
				int c = r % n[d];
				r /= n[d];
				off += node_off(G, d, lo[d] + c);
			}
			unsafeAtomicAdd(&dst[off * perNode + m], v);
		}
	}
};

template <int ND, bool V3D>
__global__ __launch_bounds__(kThreads) void k_deposit_tiled(const double *__restrict__ x0,
                                                            const double *__restrict__ x1,
                                                            const double *__restrict__ x2, long b0,
                                                            long n, pinc_geom_t g,
                                                            double *__restrict__ rho) {
	constexpr int NC = 1 << ND;
	__shared__ double acc[kDepCap];
	__shared__ BlockBounds<3, false, false> bounds;
	__shared__ int box[7];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	const ChunkItems<kDepItems> ch(b0, n);

	// pass 1: bounding box of the chunk's cells (j .. j+1 per dimension)
	int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, unused = 0;
#pragma unroll
	for (int d = 0; d < ND; d++) chunk_cell_bounds<false>(ch, xs[d], 0, lo[d], hi[d], unused);
	bounds.reduce(ND, lo, hi, nullptr, 0);
	if (threadIdx.x == 0) {
		long vol = 1;
		for (int d = 0; d < ND; d++) {
			int a, b, s;
			bounds.get(d, a, b, s);
			box[d] = a;
			box[3 + d] = b - a + 1;
			vol *= (long)(b - a + 1);
		}
		box[6] = (vol <= kDepCap && vol > 0) ? (int)vol : 0;
	}
	__syncthreads();

	NodeBox<ND> nb;
	if (box[6]) {
		nb = NodeBox<ND>(box, box + 3);
		nb.zero(acc, 1);
		__syncthreads();
	}

	// pass 2: runs of equal cells summed in registers
	int cj[3] = {INT32_MIN, 0, 0};
	double a[NC];
#pragma unroll
	for (int c = 0; c < NC; c++) a[c] = 0.0;
	auto flush = [&]() {
		if (cj[0] == INT32_MIN) return;
		if (nb.vol) {
			// (the bounding box: every run is inside)
			int l0;
			nb.index(cj, l0);
#pragma unroll
			for (int c = 0; c < NC; c++) atomicAdd(&acc[l0 + nb.corner(c)], a[c]);
		} else {
#pragma unroll
			for (int c = 0; c < NC; c++) unsafeAtomicAdd(&rho[corner_off<ND>(G, cj, c)], a[c]);
		}
	};
#pragma unroll 2
	for (int k = 0; k < kDepItems; k += 2) {
		double pp[2][3];
#pragma unroll
		for (int d = 0; d < ND; d++) ch.load2(xs[d], k, pp[0][d], pp[1][d]);
#pragma unroll
		for (int h = 0; h < 2; h++) {
			if (!ch.live(k + h)) continue;
			double dec[3], comp[3], w[NC];
			int j[3];
			const bool same = cell_split<ND, false>(pp[h], G.T, cj, j, dec, comp);
			cic_weights<ND, V3D>(dec, comp, w);
			literal_ghost_weights<ND>(g, j, w);
			if (same) {
#pragma unroll
				for (int c = 0; c < NC; c++) a[c] += w[c];
			} else {
				flush();
#pragma unroll
				for (int c = 0; c < NC; c++) a[c] = w[c];
#pragma unroll
				for (int d = 0; d < ND; d++) cj[d] = j[d];
			}
		}
	}
	flush();
	if (!nb.vol) return;
	__syncthreads();
	nb.flush(acc, 1, G, rho);
}

// ---------------------------------------------------------- moments -------
// The first velocity moments of one species on the grid (not in the
// reference; include/pinc_hip.h has the definitions): per node NM = 1 + nd +
// nd (nd + 1) / 2 sums of CIC weight times 1, v_i, v_i v_j (i <= j), value-major.
// The frame above (ChunkItems, BlockBounds, NodeBox, cell_split) with three
// differences from k_deposit_tiled (DESIGN.md "Moments"):
//  * a node is NM doubles, so the LDS box holds kMomLds / NM nodes (640 in
//    3-D, 50 KiB: three workgroups per CU).  A chunk whose cells' bounding
//    box fits uses it; otherwise the box is a fixed shape around the chunk's
//    mean cell (what a tile-sorted chunk spans after some steps of decay) and
//    the runs outside it go to global memory, so stragglers cost their own
//    atomics and not the whole chunk's LDS path;
//  * a run of particles in one cell is summed in registers for GM moments at
//    a time (2^nd GM <= 32 accumulators), in ceil(NM / GM) passes over the
//    thread's particles, which are read again (from cache) in each pass: 80
//    accumulators in one pass would not fit the register budget of two waves
//    per SIMD;
//  * the box is value-major (NodeBox with perNode = NM): its flush runs value
//    by value in storage order, so a wave's global atomics cover the
//    contiguous NM values of neighbouring nodes.
// geom.literal is ignored.  Cells are clamped to the slab (0..T_d), so that a
// particle outside the frame cannot be deposited outside the array.
constexpr int kMomItems = 16;
constexpr int kMomChunk = kThreads * kMomItems;
constexpr int kMomLds = 6400;  // doubles per workgroup
__constant__ int kMomBox[3][3] = {{2048, 1, 1}, {32, 32, 1}, {11, 7, 7}};  // nodes, by nd

template <int ND>
__global__ __launch_bounds__(kThreads) void k_moments(const double *__restrict__ x0, const double *__restrict__ x1,
                                                      const double *__restrict__ x2, const double *__restrict__ v0,
                                                      const double *__restrict__ v1, const double *__restrict__ v2,
                                                      long b0, long n, pinc_geom_t g, double *__restrict__ mom) {
	constexpr int NC = 1 << ND;
	constexpr int NM = 1 + ND + ND * (ND + 1) / 2;
	constexpr int GM = (32 / NC < NM) ? 32 / NC : NM;
	constexpr int NG = (NM + GM - 1) / GM;
	constexpr int CAP = kMomLds / NM;  // nodes of the LDS box
	static_assert(NG <= 3, "moment passes");
	__shared__ double acc[kMomLds];
	__shared__ BlockBounds<3, true, true> bounds;
	__shared__ int box[7];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	const double *vs[3] = {v0, v1, v2};
	const ChunkItems<kMomItems> ch(b0, n);

	// pass 0: bounding box and mean of the chunk's cells
	int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, sum[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) chunk_cell_bounds<true>(ch, xs[d], G.T[d], lo[d], hi[d], sum[d]);
	bounds.reduce(ND, lo, hi, sum, __popc(ch.valid));
	if (threadIdx.x == 0) {
		const int cnt = bounds.extra();
		long vol = 1;
		int a[3], b[3], m[3];
		for (int d = 0; d < ND; d++) {
			bounds.get(d, a[d], b[d], m[d]);
			vol *= (long)(b[d] - a[d] + 1);
		}
		if (cnt > 0 && vol > CAP) {
			// the fixed box around the mean cell; what lies outside goes to
			// global memory
			vol = 1;
			for (int d = 0; d < ND; d++) {
				const int e = kMomBox[ND - 1][d];
				a[d] = m[d] / cnt - (e - 2) / 2;
				b[d] = a[d] + e - 1;
				vol *= e;
			}
		}
		for (int d = 0; d < ND; d++) {
			box[d] = a[d];
			box[3 + d] = b[d] - a[d] + 1;
		}
		box[6] = cnt > 0 ? (int)vol : 0;
	}
	__syncthreads();
	if (!box[6]) return;  // (no live particle in this chunk)

	const NodeBox<ND> nb(box, box + 3);
	nb.zero(acc, NM);
	__syncthreads();

	// passes 1..NG: moments [gm * GM, gm * GM + GM) of runs of equal cells
	auto pass = [&](auto gc) {
		constexpr int M0 = decltype(gc)::value * GM;
		constexpr int MN = (M0 + GM <= NM) ? GM : NM - M0;
		int cj[3] = {INT32_MIN, 0, 0};
		double a[NC][MN];
#pragma unroll
		for (int c = 0; c < NC; c++)
#pragma unroll
			for (int q = 0; q < MN; q++) a[c][q] = 0.0;
		auto flush = [&]() {
			if (cj[0] == INT32_MIN) return;
			int l0;
			if (nb.index(cj, l0)) {
#pragma unroll
				for (int c = 0; c < NC; c++)
#pragma unroll
					for (int q = 0; q < MN; q++) atomicAdd(&acc[(l0 + nb.corner(c)) * NM + M0 + q], a[c][q]);
			} else {
#pragma unroll
				for (int c = 0; c < NC; c++) {
					double *p = mom + corner_off<ND>(G, cj, c) * NM + M0;
#pragma unroll
					for (int q = 0; q < MN; q++) unsafeAtomicAdd(p + q, a[c][q]);
				}
			}
		};
#pragma unroll 2
		for (int k = 0; k < kMomItems; k += 2) {
			double pp[2][3], pv[3][2];
#pragma unroll
			for (int d = 0; d < ND; d++) {
				ch.load2(xs[d], k, pp[0][d], pp[1][d]);
				ch.load2(vs[d], k, pv[d][0], pv[d][1]);
			}
#pragma unroll
			for (int h = 0; h < 2; h++) {
				if (!ch.live(k + h)) continue;
				double dec[3], comp[3], w[NC], f[NM];
				int j[3];
				const bool same = cell_split<ND, true>(pp[h], G.T, cj, j, dec, comp);
				cic_weights<ND, ND == 3>(dec, comp, w);
				// 1, v_i, v_i v_j (i <= j, row-major upper triangle)
				f[0] = 1.0;
				{
					int m = 1 + ND;
#pragma unroll
					for (int d = 0; d < ND; d++) f[1 + d] = pv[d][h];
#pragma unroll
					for (int d = 0; d < ND; d++)
#pragma unroll
						for (int e = d; e < ND; e++) f[m++] = pv[d][h] * pv[e][h];
				}
				if (!same) {
					flush();
#pragma unroll
					for (int c = 0; c < NC; c++)
#pragma unroll
						for (int q = 0; q < MN; q++) a[c][q] = 0.0;
#pragma unroll
					for (int d = 0; d < ND; d++) cj[d] = j[d];
				}
#pragma unroll
				for (int c = 0; c < NC; c++)
#pragma unroll
					for (int q = 0; q < MN; q++) a[c][q] += w[c] * f[M0 + q];
			}
		}
		flush();
	};
	pass(std::integral_constant<int, 0>{});
	if constexpr (NG > 1) pass(std::integral_constant<int, 1>{});
	if constexpr (NG > 2) pass(std::integral_constant<int, 2>{});
	__syncthreads();
	nb.flush(acc, NM, G, mom);
}

// ------------------------------------------------------ phase space -------
// Histogram of one species over NA = 1 or 2 of its coordinates (not in the
// reference; include/pinc_hip.h has the binning rule).  Of the frame above it
// uses ChunkItems, on the one or two arrays the spec names, and BlockBounds;
// its counters are bins, not nodes, so the box is its own.
//  * pass 0 bins the thread's particles (the bins stay in registers) and
//    finds the chunk's bounding box in bin space from the inside particles;
//  * a box of at most kPhLds bins is counted in LDS with 32-bit counters (a
//    chunk has 4096 particles: no overflow) and flushed with one 64-bit
//    global atomic per non-zero counter.  A small box is kept in up to
//    kPhCopies copies, lane & (copies - 1) picks one (odd stride: the copies
//    of a bin lie in different banks), as the push keeps its charge box: f(v)
//    puts most of a wave into a few bins, and same-address LDS atomics
//    serialise inside a wave.  The flush sums the copies;
//  * a box that does not fit: one 64-bit global atomic per inside particle.
// Outside particles are counted per thread, summed per wave and added with
// one atomic per workgroup.
constexpr int kPhItems = 16;
constexpr int kPhChunk = kThreads * kPhItems;
// Measured at 128^3, 64 ppc (tools/phase_probe.py, profiles/phase_space.json):
// 4096, 8192 and 16384 counters take 7.73, 6.94 and 6.21 ms over the six
// probed cases (16384 halves (x, vx) after 8 steps without a sort, 1.99 ->
// 0.99 ms, and costs 0.1 ms where 8192 already fits); 1, 4, 8 or 16 copies
// are within the noise of each other (f(vx) 0.92-0.94 ms: its time is the
// flush's atomics of every workgroup into the same 128 bins, not the LDS).
constexpr int kPhLds = 16384;  // 32-bit counters of the LDS box (64 KiB: two workgroups per CU)
constexpr int kPhCopies = 8;   // as the push's charge box

template <int NA>
__global__ __launch_bounds__(kThreads) void k_phase_hist(const double *__restrict__ c0, const double *__restrict__ c1,
                                                         long b0, long n, pinc_phase_t sp,
                                                         unsigned long long *__restrict__ hist,
                                                         unsigned long long *__restrict__ outside) {
	__shared__ unsigned cnt[kPhLds + 1];
	__shared__ BlockBounds<NA, false, true> bounds;
	__shared__ int box[6];
	const double *cs[2] = {c0, c1};
	const ChunkItems<kPhItems> ch(b0, n);
	const int lane = threadIdx.x & 63;

	// pass 0: the bins, and the chunk's bounding box of the inside particles
	int bin[NA][kPhItems];
	unsigned in = ch.valid;
#pragma unroll
	for (int a = 0; a < NA; a++) {
		const double shift = sp.shift[a], lo = sp.lo[a], scale = sp.scale[a], nb = (double)sp.nbins[a];
#pragma unroll
		for (int k = 0; k < kPhItems; k += 2) {
			double c[2];
			ch.load2(cs[a], k, c[0], c[1]);
#pragma unroll
			for (int h = 0; h < 2; h++) {
				const double t = ((c[h] + shift) - lo) * scale;
				const bool ok = t >= 0.0 && t < nb;
				bin[a][k + h] = ok ? (int)t : 0;
				if (!ok) in &= ~(1u << (k + h));
			}
		}
	}
	int lo[NA], hi[NA];
#pragma unroll
	for (int a = 0; a < NA; a++) {
		lo[a] = INT32_MAX, hi[a] = INT32_MIN;
#pragma unroll
		for (int k = 0; k < kPhItems; k++)
			if ((in >> k) & 1u) {
				lo[a] = min(lo[a], bin[a][k]);
				hi[a] = max(hi[a], bin[a][k]);
			}
	}
	bounds.reduce(NA, lo, hi, nullptr, __popc(ch.valid & ~in));
	if (threadIdx.x == 0) {
		const int out = bounds.extra();
		if (out) atomicAdd(outside, (unsigned long long)out);
		long area = 1;
		bool any = true;
		box[1] = 0, box[3] = 1;
		for (int a = 0; a < NA; a++) {
			int x, y, s;
			bounds.get(a, x, y, s);
			any = any && y >= x;
			if (!any) break;
			box[a] = x;
			box[2 + a] = y - x + 1;
			area *= (long)(y - x + 1);
		}
		// 0: no inside particle; -1: the box does not fit; else its area
		box[4] = !any ? 0 : area <= kPhLds ? (int)area : -1;
		int nc = 1;
		if (any && area <= kPhLds)
			while (nc < kPhCopies && 2 * nc * ((int)area | 1) <= kPhLds + 1) nc *= 2;
		box[5] = nc;
	}
	__syncthreads();
	const int area = box[4];
	if (!area) return;
	const long nb0 = sp.nbins[0];
	if (area < 0) {
#pragma unroll
		for (int k = 0; k < kPhItems; k++)
			if ((in >> k) & 1u) atomicAdd(&hist[(NA > 1 ? bin[NA - 1][k] * nb0 : 0L) + bin[0][k]], 1ull);
		return;
	}
	const int lo0 = box[0], lo1 = box[1], w0 = box[2], nCopy = box[5];
	const int stride = area | 1;
	const int mine = (lane & (nCopy - 1)) * stride;
	for (int t = threadIdx.x; t < nCopy * stride; t += kThreads) cnt[t] = 0u;
	__syncthreads();
#pragma unroll
	for (int k = 0; k < kPhItems; k++)
		if ((in >> k) & 1u) atomicAdd(&cnt[mine + (NA > 1 ? (bin[NA - 1][k] - lo1) * w0 : 0) + (bin[0][k] - lo0)], 1u);
	__syncthreads();
	for (int t = threadIdx.x; t < area; t += kThreads) {
		unsigned v = cnt[t];
		for (int c = 1; c < nCopy; c++) v += cnt[c * stride + t];
		if (!v) continue;
		const int r1 = t / w0, r0 = t - r1 * w0;
		atomicAdd(&hist[(lo1 + r1) * nb0 + lo0 + r0], (unsigned long long)v);
	}
}

// ------------------------------------------------------- accelerate -------
// puAcc3D1KE / puAccND1KE.  The reference rescales the whole E grid per
// species (gMul(E,q/m) ... gMul(E,m/q), pusher.c:192,212); k_field_chain
// materialises E as it stands while species s is pushed (same rounding
// chain), so the particle kernel gathers plain values.  Particles are loaded
// and stored as lane-contiguous 16-B pairs; the gathered corner values are
// reused while a thread's next particle stays in the same cell.
constexpr int kAccItems = 8;
constexpr int kAccChunk = kThreads * kAccItems;

__global__ void k_field_chain(const double *__restrict__ E, double *__restrict__ Es, long n,
                              const double *__restrict__ qm, const double *__restrict__ mq,
                              double pre, int s) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
		double v = E[i] * pre;
		for (int t = 0; t < s; t++) v = (v * qm[t]) * mq[t];
		Es[i] = v * qm[s];
	}
}

// every species' rescaled copy of E in one pass over E (k_field_chain's
// chain for species s is species s-1's times mq[s-1] qm[s] / qm[s-1]... in
// the same expression order: the running v of the loop above), species s at
// Es + s n
__global__ void k_field_chain_all(const double *__restrict__ E, double *__restrict__ Es, long n,
                                  const double *__restrict__ qm, const double *__restrict__ mq, double pre,
                                  int nSpecies) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
		double v = E[i] * pre;
		Es[i] = v * qm[0];
		for (int s = 1; s < nSpecies; s++) {
			v = (v * qm[s - 1]) * mq[s - 1];
			Es[(long)s * n + i] = v * qm[s];
		}
	}
}

// Boris rotation parameters of one species (puGet3DRotationParameters,
// pusher.c:485-505)
struct BorisRot {
	double T[3], S[3];
};

// v x b added to res in addCross's expression order (pusher.c:1234-1238)
__device__ __forceinline__ void add_cross(const double *a, const double *b, double *res) {
	res[0] += (a[1] * b[2] - a[2] * b[1]);
	res[1] += -(a[0] * b[2] - a[2] * b[0]);
	res[2] += (a[0] * b[1] - a[1] * b[0]);
}

template <int ND, bool V3D, bool KE, bool BORIS = false>
__global__ __launch_bounds__(kThreads) void k_accel(const double *__restrict__ x0,
                                                    const double *__restrict__ x1,
                                                    const double *__restrict__ x2,
                                                    double *__restrict__ v0, double *__restrict__ v1,
                                                    double *__restrict__ v2, long b0, long n,
                                                    pinc_geom_t g, const double *__restrict__ E,
                                                    double *__restrict__ kePartial, BorisRot rot = {}) {
	constexpr int NC = 1 << ND;
	__shared__ double red[kThreads / 64];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	double *vs[3] = {v0, v1, v2};
	const long end = b0 + n;
	// pair k/2 of the lane-contiguous pairs (1 KiB per wave load instruction)
	const long cb = (b0 & ~1L) + (long)blockIdx.x * kAccChunk + 2L * threadIdx.x;
	double ke = 0.;
	int cj[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
	double e[NC][ND];  // corner values of the current cell
#pragma unroll
	for (int k = 0; k < kAccItems; k += 2) {
		double p[3][2], v[3][2];
		bool ok[2];
		ok[0] = (cb + 2L * kThreads * (k >> 1) >= b0) && (cb + 2L * kThreads * (k >> 1) < end);
		ok[1] = (cb + 2L * kThreads * (k >> 1) + 1 >= b0) && (cb + 2L * kThreads * (k >> 1) + 1 < end);
		if (!ok[0] && !ok[1]) continue;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			if (ok[0] && ok[1]) {
				double2 a = *reinterpret_cast<const double2 *>(xs[d] + cb + 2L * kThreads * (k >> 1));
				double2 b = *reinterpret_cast<const double2 *>(vs[d] + cb + 2L * kThreads * (k >> 1));
				p[d][0] = a.x;
				p[d][1] = a.y;
				v[d][0] = b.x;
				v[d][1] = b.y;
			} else {
				long i = ok[0] ? cb + 2L * kThreads * (k >> 1) : cb + 2L * kThreads * (k >> 1) + 1;
				int h = ok[0] ? 0 : 1;
				p[d][h] = xs[d][i];
				v[d][h] = vs[d][i];
				p[d][1 - h] = p[d][h];
				v[d][1 - h] = v[d][h];
			}
		}
#pragma unroll
		for (int h = 0; h < 2; h++) {
			if (!ok[h]) continue;
			double dec[3], comp[3];
			int j[3];
			bool same = true;
#pragma unroll
			for (int d = 0; d < ND; d++) {
				j[d] = (int)p[d][h];
				dec[d] = p[d][h] - j[d];
				comp[d] = 1 - dec[d];
				same = same && (j[d] == cj[d]);
			}
			if (!same) {
#pragma unroll
				for (int c = 0; c < NC; c++) {
					long off = 0;
#pragma unroll
					for (int d = 0; d < ND; d++) off += node_off(G, d, j[d] + ((c >> d) & 1));
					off *= ND;
#pragma unroll
					for (int q = 0; q < ND; q++) e[c][q] = E[off + q];
				}
#pragma unroll
				for (int d = 0; d < ND; d++) cj[d] = j[d];
			}
			double dv[ND];
			if (V3D) {
				// puInterp3D1 (pusher.c:1116-1120), corner c = x + 2y + 4z
				double x = dec[0], y = dec[1], z = dec[2];
				double xc = comp[0], yc = comp[1], zc = comp[2];
#pragma unroll
				for (int q = 0; q < ND; q++)
					dv[q] = zc * (yc * (xc * e[0][q] + x * e[1][q]) + y * (xc * e[2][q] + x * e[3][q])) +
					        z * (yc * (xc * e[4][q] + x * e[5][q]) + y * (xc * e[6][q] + x * e[7][q]));
			} else {
				// puInterpND1Inner: corner by corner in the recursion order
				// (outer dims first), (c_x*f)*val
#pragma unroll
				for (int q = 0; q < ND; q++) dv[q] = 0;
#pragma unroll
				for (int c = 0; c < (1 << (ND - 1)); c++) {
					double f = 1.0;
					int cc = 0;
#pragma unroll
					for (int d = ND - 1; d >= 1; d--) {
						int bit = (c >> (d - 1)) & 1;
						f = (bit ? dec[d] : comp[d]) * f;
						cc |= bit << d;
					}
#pragma unroll
					for (int q = 0; q < ND; q++) {
						dv[q] += comp[0] * f * e[cc][q];
						dv[q] += dec[0] * f * e[cc | 1][q];
					}
				}
			}
			double vsq = 0;
			if constexpr (BORIS) {
				// puBoris3D1KE (pusher.c:455-476) with the indexing corrected:
				// half kick, rotation about B, KE of v+, half kick
				double vm[3], vp[3];
#pragma unroll
				for (int d = 0; d < 3; d++) vm[d] = v[d][h] + 0.5 * dv[d];
#pragma unroll
				for (int d = 0; d < 3; d++) vp[d] = vm[d];
				add_cross(vm, rot.T, vp);
				add_cross(vp, rot.S, vm);
#pragma unroll
				for (int d = 0; d < 3; d++) vsq += vm[d] * vm[d];
#pragma unroll
				for (int d = 0; d < 3; d++) v[d][h] = vm[d] + 0.5 * dv[d];
			} else {
#pragma unroll
				for (int d = 0; d < ND; d++) {
					double vv = v[d][h];
					vsq += vv * (vv + dv[d]);
					v[d][h] = vv + dv[d];
				}
			}
			ke += vsq;
		}
#pragma unroll
		for (int d = 0; d < ND; d++) {
			if (ok[0] && ok[1]) {
				*reinterpret_cast<double2 *>(vs[d] + cb + 2L * kThreads * (k >> 1)) = make_double2(v[d][0], v[d][1]);
			} else {
				if (ok[0]) vs[d][cb + 2L * kThreads * (k >> 1)] = v[d][0];
				if (ok[1]) vs[d][cb + 2L * kThreads * (k >> 1) + 1] = v[d][1];
			}
		}
	}
	if (KE) {
		double t = block_sum(ke, red);
		if (threadIdx.x == 0) kePartial[blockIdx.x] = t;
	}
}

// ------------------------------------------------------------- init -------
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
	z += 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}
__device__ __forceinline__ double uni(unsigned long long seed, unsigned long long c) {
	unsigned long long x = mix64(seed ^ mix64(c));
	return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double normal(unsigned long long seed, unsigned long long c) {
	double u1 = uni(seed, 2 * c), u2 = uni(seed, 2 * c + 1);
	return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

struct LatticeArgs {
	int nd;
	int L[3];
	int sub[3];
	int off[3];
	double posToSub[3];
	double l;
	double amp[3], mode[3];
	int perturb, maxwell;
	double drift, vth;
	unsigned long long seed;
	int species;
};

__device__ __forceinline__ bool lattice_pos(const LatticeArgs &a, long i, double *x) {
	double lin = a.l * (double)i;
	for (int d = 0; d < a.nd; d++) {
		x[d] = fmod(lin, (double)a.L[d]);
		lin /= a.L[d];
	}
	int ok = 0;
	for (int d = 0; d < a.nd; d++) ok += (a.sub[d] == (int)(a.posToSub[d] * x[d]));
	return ok == a.nd;
}

__global__ __launch_bounds__(kThreads) void k_lattice_count(LatticeArgs a, long nGlobal,
                                                            int *__restrict__ chunkCount) {
	__shared__ int wcnt[kThreads / 64];
	long base = (long)blockIdx.x * PINC_CHUNK;
	int cnt = 0;
	for (int k = 0; k < kItems; k++) {
		long i = base + k * kThreads + threadIdx.x;
		double x[3];
		if (i < nGlobal && lattice_pos(a, i, x)) cnt++;
	}
	int ws = wave_sum(cnt);
	if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = ws;
	__syncthreads();
	if (threadIdx.x == 0) {
		int t = 0;
		for (int q = 0; q < kThreads / 64; q++) t += wcnt[q];
		chunkCount[blockIdx.x] = t;
	}
}

__global__ __launch_bounds__(kThreads) void k_lattice_write(LatticeArgs a, long nGlobal,
                                                            const int *__restrict__ chunkOffset,
                                                            pinc_pop_t pop, long sbase) {
	__shared__ int wtot[kThreads / 64];
	long base = (long)blockIdx.x * PINC_CHUNK;
	int running = chunkOffset[blockIdx.x];
	int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	for (int k = 0; k < kItems; k++) {
		long i = base + k * kThreads + threadIdx.x;
		double x[3] = {0, 0, 0};
		bool keep = i < nGlobal && lattice_pos(a, i, x);
		unsigned long long b = __ballot(keep);
		int rw = __popcll(b & lanemask_lt());
		if (lane == 0) wtot[w] = __popcll(b);
		__syncthreads();
		int before = 0, tot = 0;
		for (int q = 0; q < kThreads / 64; q++) {
			before += (q < w) ? wtot[q] : 0;
			tot += wtot[q];
		}
		if (keep) {
			long dst = sbase + running + before + rw;
			for (int d = 0; d < a.nd; d++) {
				double p = x[d];  // global frame
				if (a.perturb) {
					double theta = 2.0 * M_PI * a.mode[d] * p / a.L[d];
					p += a.amp[d] * cos(theta);
				}
				pop.x[d][dst] = p - a.off[d];
				double v = 0.0;
				if (a.maxwell) {
					unsigned long long c =
						(((unsigned long long)a.species << 40) | (unsigned long long)i) * 3ULL + d;
					v = a.drift + a.vth * normal(a.seed, c);
				}
				pop.v[d][dst] = v;
			}
		}
		running += tot;
		__syncthreads();
	}
}

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }


// ----------------------------------------------------- tiled layout -------
// Counting sort of one species by tile (a TW^nd block of cells) for the
// optional tiled layout (population:layout = tiled).  Particles of a tile
// become contiguous, so a deposit or gather chunk touches a few hundred
// nodes instead of whole rows.  Within a tile the order is arbitrary.
struct TileGeo {
	int tw;         // cells per tile side
	int nt[3];      // tiles per dimension (cell index (int)p is in [0, T+1])
	int cmax[3];    // largest admissible cell index
	// bricks of the push's sort: tw^(nd-1) consecutive cell keys of a tile
	// (tw x tw x 1 in 3-D), bs[d] = log2 of the brick's extent along d (all
	// 0: bricks of one cell)
	int bs[3];
};

// Sort key: tile index, then the cell inside the tile.  Tiles run along a
// serpentine (x rows alternate direction, y columns alternate per z plane),
// and a tile's layers along the slab dimension run in reverse in odd tiles,
// so consecutive keys of different tiles are neighbouring cells: a block of
// particles that straddles two tiles after a sort spans two adjacent bricks
// (8 x 4 x 1 cells), not a jump of a whole tile row or of the tile's depth.
// Inside a layer the cells are x fastest, so a brick (one layer of a tile,
// TileGeo::bs) is a run of consecutive keys.
template <int ND>
__device__ __forceinline__ long tile_serp(const TileGeo &tg, const int *t) {
	if (ND == 1) return t[0];
	if (ND == 2) return (long)t[1] * tg.nt[0] + ((t[1] & 1) ? tg.nt[0] - 1 - t[0] : t[0]);
	const int ty = (t[2] & 1) ? tg.nt[1] - 1 - t[1] : t[1];
	const long r = (long)t[2] * tg.nt[1] + ty;
	return r * tg.nt[0] + ((r & 1) ? tg.nt[0] - 1 - t[0] : t[0]);
}
// inverse of tile_serp
template <int ND>
__device__ __forceinline__ void tile_unserp(const TileGeo &tg, long tile, int *t) {
	t[1] = t[2] = 0;
	if (ND == 1) {
		t[0] = (int)tile;
		return;
	}
	const long r = tile / tg.nt[0];
	const int tx = (int)(tile - r * tg.nt[0]);
	t[0] = (r & 1) ? tg.nt[0] - 1 - tx : tx;
	if (ND == 2) {
		t[1] = (int)r;
		return;
	}
	t[2] = (int)(r / tg.nt[1]);
	const int ty = (int)(r - (long)t[2] * tg.nt[1]);
	t[1] = (t[2] & 1) ? tg.nt[1] - 1 - ty : ty;
}
// key of clamped cell coordinates c (each in [0, cmax])
template <int ND>
__device__ __forceinline__ int tile_key_of(const TileGeo &tg, const int *c) {
	int t[3] = {0, 0, 0}, in[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		t[d] = c[d] / tg.tw;
		in[d] = c[d] - t[d] * tg.tw;
	}
	const long tile = tile_serp<ND>(tg, t);
	if (ND > 1 && (tile & 1)) in[ND - 1] = tg.tw - 1 - in[ND - 1];
	int cell = 0, cs = 1;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		cell += in[d] * cs;
		cs *= tg.tw;
	}
	return (int)(tile * cs + cell);
}
// cell coordinates of a key (inverse of tile_key_of)
template <int ND>
__device__ __forceinline__ void tile_key_cell(const TileGeo &tg, long key, int *c) {
	int cpt = 1;
#pragma unroll
	for (int d = 0; d < ND; d++) cpt *= tg.tw;
	const long tile = key / cpt;
	int in = (int)(key - tile * cpt);
	int t[3];
	tile_unserp<ND>(tg, tile, t);
	c[1] = c[2] = 0;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		int q = in % tg.tw;
		in /= tg.tw;
		if (ND > 1 && d == ND - 1 && (tile & 1)) q = tg.tw - 1 - q;
		c[d] = t[d] * tg.tw + q;
	}
}
template <int ND>
__device__ __forceinline__ int tile_key(const TileGeo &tg, const double *p) {
	int c[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		const int x = (int)p[d];
		c[d] = x < 0 ? 0 : (x > tg.cmax[d] ? tg.cmax[d] : x);
	}
	return tile_key_of<ND>(tg, c);
}

// wave-aggregated atomicAdd of 1 per active lane on ctr[key]; returns the
// lane's slot (old value + rank among the lanes with the same key)
__device__ __forceinline__ int agg_add(int *ctr, int key, bool active) {
	int lane = threadIdx.x & 63;
	unsigned long long pending = __ballot(active);
	int mine = 0;
	while (pending) {
		int leader = __ffsll((long long)pending) - 1;
		int lk = __shfl(key, leader, 64);
		unsigned long long m = __ballot(active && key == lk) & pending;
		int base = 0;
		if (lane == leader) base = atomicAdd(&ctr[lk], __popcll(m));
		base = __shfl(base, leader, 64);
		if ((m >> lane) & 1ull) mine = base + __popcll(m & lanemask_lt());
		pending &= ~m;
	}
	return mine;
}

template <int ND>
__global__ __launch_bounds__(kThreads) void k_sort_count(const double *__restrict__ x0,
                                                         const double *__restrict__ x1,
                                                         const double *__restrict__ x2, long n,
                                                         TileGeo tg, int *__restrict__ counts) {
	const double *xs[3] = {x0, x1, x2};
	for (long base = (long)blockIdx.x * blockDim.x; base < n; base += (long)gridDim.x * blockDim.x) {
		long i = base + threadIdx.x;
		bool act = i < n;
		double p[3] = {0, 0, 0};
		if (act) {
#pragma unroll
			for (int d = 0; d < ND; d++) p[d] = xs[d][i];
		}
		int key = act ? tile_key<ND>(tg, p) : 0;
		agg_add(counts, key, act);
	}
}

// the sorting push's key counts: per brick, at the brick's first key (the
// push reserves per brick; immigrants joining the counts, or counts made
// without a counting push)
// Cell a particle is sorted by in the in-push sort (the counting push, the
// brick counts and the sorting push must agree): the cell of x + v, where
// the next push's drift takes it before its kick, so that a sorting push's
// output lies in the bricks it was ranked into (sorted by the input cell x,
// the output of every block spread one cell around its bricks: E and charge
// boxes 6 x 6 x 3 cells instead of 4 x 4 x 1).  Clamped to the grid like
// every key (a particle that wraps through a periodic face is placed at the
// face it left: order only).
__device__ __forceinline__ int sort_cell(double x, double v) { return (int)(x + v); }

template <int ND>
__global__ __launch_bounds__(kThreads) void k_count_bricks(const double *__restrict__ x0,
                                                           const double *__restrict__ x1,
                                                           const double *__restrict__ x2,
                                                           const double *__restrict__ v0,
                                                           const double *__restrict__ v1,
                                                           const double *__restrict__ v2, long n,
                                                           TileGeo tg, int *__restrict__ counts) {
	const double *xs[3] = {x0, x1, x2}, *vs[3] = {v0, v1, v2};
	for (long base = (long)blockIdx.x * blockDim.x; base < n; base += (long)gridDim.x * blockDim.x) {
		long i = base + threadIdx.x;
		bool act = i < n;
		int c[3] = {0, 0, 0};
		if (act) {
#pragma unroll
			for (int d = 0; d < ND; d++) c[d] = sort_cell(xs[d][i], vs[d][i]);
		}
		agg_add(counts, act ? brick_first_key<ND>(tg, c) : 0, act);
	}
}

template <int ND>
__global__ __launch_bounds__(kThreads) void k_sort_scatter(pinc_pop_t in, pinc_pop_t out, long b0, long n,
                                                           TileGeo tg, int *__restrict__ cursor) {
	for (long base = (long)blockIdx.x * blockDim.x; base < n; base += (long)gridDim.x * blockDim.x) {
		long i = base + threadIdx.x;
		bool act = i < n;
		double p[3] = {0, 0, 0}, v[3] = {0, 0, 0};
		if (act) {
#pragma unroll
			for (int d = 0; d < ND; d++) {
				p[d] = in.x[d][b0 + i];
				v[d] = in.v[d][b0 + i];
			}
		}
		int key = act ? tile_key<ND>(tg, p) : 0;
		int slot = agg_add(cursor, key, act);
		if (act) {
#pragma unroll
			for (int d = 0; d < ND; d++) {
				out.x[d][b0 + slot] = p[d];
				out.v[d][b0 + slot] = v[d];
			}
		}
	}
}


// exclusive scan of n ints for large n: block sums, a single-block scan of
// those, then per-block scans with the block offsets; out[n] = total
constexpr int kScanItems = 16;
constexpr int kScanBlock = kThreads * kScanItems;

__global__ __launch_bounds__(kThreads) void k_scan_sums(const int *__restrict__ in, long n,
                                                        int *__restrict__ sums) {
	__shared__ int w[kThreads / 64];
	long b0 = (long)blockIdx.x * kScanBlock;
	int t = 0;
	for (int k = 0; k < kScanItems; k++) {
		long i = b0 + (long)k * kThreads + threadIdx.x;
		if (i < n) t += in[i];
	}
	t = wave_sum(t);
	if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = t;
	__syncthreads();
	if (threadIdx.x == 0) {
		int s = 0;
		for (int q = 0; q < kThreads / 64; q++) s += w[q];
		sums[blockIdx.x] = s;
	}
}

__global__ __launch_bounds__(kThreads) void k_scan_apply(const int *__restrict__ in, long n,
                                                         const int *__restrict__ offs,
                                                         int *__restrict__ out) {
	__shared__ int wtot[kThreads / 64];
	long b0 = (long)blockIdx.x * kScanBlock;
	// thread owns kScanItems consecutive elements
	long i0 = b0 + (long)threadIdx.x * kScanItems;
	int v[kScanItems];
	int t = 0;
#pragma unroll
	for (int k = 0; k < kScanItems; k++) {
		v[k] = (i0 + k < n) ? in[i0 + k] : 0;
		t += v[k];
	}
	// exclusive scan of t over the block
	int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	int x = t;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		int y = __shfl_up(x, o, 64);
		if (lane >= o) x += y;
	}
	if (lane == 63) wtot[wv] = x;
	__syncthreads();
	int before = 0;
	for (int q = 0; q < wv; q++) before += wtot[q];
	int run = offs[blockIdx.x] + before + x - t;
#pragma unroll
	for (int k = 0; k < kScanItems; k++) {
		if (i0 + k < n) out[i0 + k] = run;
		run += v[k];
	}
	if (i0 + kScanItems >= n && i0 < n) out[n] = run;
}


// ------------------------------------------ deposit over sorted cell ranges --
// Tiled layout after a sort: offs is the sort's cursor array after the
// scatter, i.e. the exclusive end of each key's range, so [offs[key-1],
// offs[key]) holds the particles that were in cell `key` at the last sort.  One thread per cell
// sums the eight CIC weights of its particles in registers (no atomics per
// particle); particles that have since moved to another cell are added
// individually (LDS box with a one-cell margin, else global atomics).  A
// workgroup covers 256 consecutive keys (4 tiles in 3-D), accumulated in LDS
// and flushed once.
template <int ND, bool V3D>
__global__ __launch_bounds__(kThreads) void k_deposit_cells(const double *__restrict__ x0,
                                                            const double *__restrict__ x1,
                                                            const double *__restrict__ x2, long nCell,
                                                            const int *__restrict__ offs, long nKeys,
                                                            TileGeo tg, pinc_geom_t g,
                                                            double *__restrict__ rho) {
	constexpr int NC = 1 << ND;
	__shared__ double acc[kDepCap];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	int cpt = 1;
#pragma unroll
	for (int d = 0; d < ND; d++) cpt *= tg.tw;
	const long k0 = (long)blockIdx.x * kThreads;
	const long k1 = min(k0 + kThreads, nKeys) - 1;
	// node box of the block's tiles plus a one-cell margin (the tiles of a
	// key range are a path of neighbouring tiles, tile_serp)
	const long t0 = k0 / cpt, t1 = k1 / cpt;
	int tlo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, thi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
	for (long t = t0; t <= t1; t++) {
		int tc[3];
		tile_unserp<ND>(tg, t, tc);
#pragma unroll
		for (int d = 0; d < ND; d++) {
			tlo[d] = min(tlo[d], tc[d]);
			thi[d] = max(thi[d], tc[d]);
		}
	}
	const bool boxOk = t1 - t0 < 16;
	int blo[3] = {0, 0, 0}, bn[3] = {1, 1, 1};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		int clo = tlo[d] * tg.tw, chi = min(thi[d] * tg.tw + tg.tw - 1, tg.cmax[d]);
		blo[d] = clo - 1;
		bn[d] = chi - clo + 4;  // nodes clo-1 .. chi+2
	}
	NodeBox<ND> nb(blo, bn);
	if (!boxOk || nb.vol > kDepCap) nb.vol = 0;
	nb.zero(acc, 1);
	__syncthreads();

	auto add8 = [&](const int *j, const double *w) {
		int l0;
		const bool inBox = nb.index(j, l0);
		if (nb.vol > 0 && inBox) {
#pragma unroll
			for (int c = 0; c < NC; c++) atomicAdd(&acc[l0 + nb.corner(c)], w[c]);
		} else {
#pragma unroll
			for (int c = 0; c < NC; c++) unsafeAtomicAdd(&rho[corner_off<ND>(G, j, c)], w[c]);
		}
	};

	const long key = k0 + threadIdx.x;
	if (key < nKeys) {
		// this thread's cell
		int cell[3] = {0, 0, 0};
		tile_key_cell<ND>(tg, key, cell);
		long a = key > 0 ? (long)offs[key - 1] : 0, b = min((long)offs[key], nCell);
		double sum[NC];
#pragma unroll
		for (int c = 0; c < NC; c++) sum[c] = 0.0;
		bool any = false;
		for (long i = a; i < b; i++) {
			double p[3], dec[3], comp[3], w[NC];
			int j[3];
#pragma unroll
			for (int d = 0; d < ND; d++) p[d] = xs[d][i];
			const bool own = cell_split<ND, false>(p, G.T, cell, j, dec, comp);
			cic_weights<ND, V3D>(dec, comp, w);
			literal_ghost_weights<ND>(g, j, w);
			if (own) {
#pragma unroll
				for (int c = 0; c < NC; c++) sum[c] += w[c];
				any = true;
			} else {
				add8(j, w);
			}
		}
		if (any) add8(cell, sum);
	}
	if (!nb.vol) return;
	__syncthreads();
	nb.flush(acc, 1, G, rho);
}

// ------------------------------------------------------- fused push -------
// One pass over a species: [kick: puAcc gather + v += dv + KE (pusher.c:
// 178-265, 1089-1162)] then drift: puMove (pusher.c:86-119) + the neighbour
// test of puExtractEmigrants (pusher.c:782-910) + puDistr of every particle
// that stays (pusher.c:512-638).  Particles that emigrate are deposited after
// their import (distr's immigrant pass), so the charge is the reference's.
//
// Thread t of block b owns particles b*2048 + k*256 + t (k = 0..7): every
// wave load and store is one contiguous 512-B run.  In a cell-ordered layout
// the 64 particles of a wave share one or two cells, so the deposit first
// reduces each large same-cell group across the wave (a transposed butterfly
// that leaves corner c's sum in lane 8c) and adds it once; the other lanes
// (particles that changed cell, sparse groups) add their own eight weights.
// Adds go to an LDS box of the block's cells (ds_add_f64), flushed with one
// global atomic per touched node; a block whose box exceeds the LDS tile adds
// to global memory directly.  Only the summation order differs from the
// serial loop.
struct PushArgs {
	const double *xi[3];
	double *xo[3];       // may alias xi (unsorted)
	const double *vi[3];
	double *vo[3];       // may alias vi (unsorted)
	long n;              // particles of the species; pointers start at it
	pinc_geom_t g;
	const double *Es;    // kick: E as rescaled for the species (k_field_chain)
	double *rho;         // species charge accumulator (slab layout)
	Thr thr;
	int center, wrapMask;
	double maxVel;
	unsigned char *flags;
	int *chunkCount;
	int *err;
	double *kePartial;
	// sorted output (tiled layout): particle i goes to cursor[key(x_i)]++,
	// the keys of the moved particles are counted in cntNext for the next push
	TileGeo tg;
	int *cursor;
	int *cntNext;
	unsigned long long *moved;  // += particles that stay but changed cell (nullable)
	unsigned long long *spread;  // += the block's input cell-box volume (nullable)
	unsigned long long *tstamp;  // 8 phase timestamps per block (diagnostics, nullable)
	unsigned long long *diag;    // [0] += sorting-push items given a global slot one by one (nullable)
	const unsigned char *objIn;  // object ids of the padded nodes (nullable: no objects)
	long objSy, objSz, objN;
	int *objCount;
	int objLo[3], objExt[3];     // bounding box of the object nodes: lower corner, extent - 1
	unsigned long long *emigTotal;  // += particles flagged to leave (nullable)
	int flagsSparse;                // only the non-centre flags are written
};
// phase timestamp of the block (thread 0, s_memrealtime at 100 MHz)
#define PUSH_TS(slot) \
	if (a.tstamp && threadIdx.x == 0) a.tstamp[(long)chunk * 8 + (slot)] = tsub = wall_clock64()
// sub-phase of the sorting push since the last PUSH_TS / PUSH_SUB, summed over
// the blocks into diag[k] (trace mode)
#define PUSH_SUB(k)                                                           \
	if (a.tstamp && threadIdx.x == 0) {                                       \
		const unsigned long long now = wall_clock64();                        \
		atomicAdd(&a.diag[k], now - tsub);                                    \
		tsub = now;                                                           \
	}

// The deposit goes into per-lane-group copies of the LDS charge box (lane &
// (nc-1) picks the copy, nc <= kPushCopies copies as the box allows) with
// plain LDS atomics.  Measured at C4 (mean over the sort cycle): same-cell
// wave reductions and no copies 29.6 ms per species launch, 2 copies 30.0,
// 4 copies 28.2, 8 copies 28.2 -- a sorted wave's lanes mostly share one
// cell, and 8 copies cut the same-address conflicts of each ds_add_f64 to
// 8-way for ~60 fewer VALU instructions per particle than the reduction.
// (Tried and rejected the same day: whole-chunk launches without per-element
// conditions, 43 ms, spills; 2 items per thread at 4-5 waves/SIMD, 31-32 ms;
// 512-thread blocks, 35.8 ms.)
constexpr int kPushCopies = 8;
constexpr int kRhoLds = 2048;  // charge box and its copies (doubles of LDS; the sorting push keeps 1024)
// 8 waves x 4 particles per thread per PINC_CHUNK block: fewer live VGPRs
// (px) than 4 waves x 8, so more waves per SIMD hide the gather latency.
// A thread's particles are consecutive in memory (measured at C4, mean over
// the sort cycle, per species launch: 27.1 ms against 28.3 for lane pairs 512
// apart), and a full block's particle loads and stores are contiguous per
// wave instruction, rows of 16 lanes swapping halves (k_push, phase A): a
// mapping where a thread loads its own four (every other 16 B of 2 KB per
// instruction) copies at 5.69 TB/s on this chip against 6.13 TB/s contiguous
// (profiles/r06b_copy_probe3_lane_mapping.jsonl).  Every wave instruction of
// a full block covers whole lines, so its particle loads and stores are
// nontemporal: plain push 19.63 -> 19.06 ms per species launch at C4, loads
// alone 19.39, stores alone 19.30 (profiles/r06g_push_nontemporal_ab.txt).
constexpr int kPushThreads = 256;
constexpr int kPushItems = 4;  // particles per thread, consecutive
constexpr int kPushWavesPerEu = 4;  // k_push's amdgpu_waves_per_eu
constexpr int kPushChunk = kPushThreads * kPushItems;  // particles per block (PINC_CHUNK / 2)
// chunks per piece of push_chunk_of's round-robin over the XCDs
constexpr unsigned kPushXcdPiece = 64;
// The sorting push orders each brick's run by cell (per (brick, cell) counters
// for blocks whose brick box holds at most kCellRankBricks bricks of at most
// 16 cells), so repeated sorts keep a brick's particles cell-contiguous
constexpr int kCellRankBricks = 64;
static_assert(kPushChunk >= PINC_CHUNK / 8 && PINC_CHUNK % kPushChunk == 0, "kePartial holds PINC_CHUNK/8 per chunk");

// storage offsets (in nodes, 32-bit) of padded node coordinates j and j+1
// along dimension d of the slab (periodic x/y stored without ghosts)
struct Geo32 {
	int T[3];
	int stride[3];
	int slab;
};
__device__ __forceinline__ Geo32 make_geo32(const pinc_geom_t &g) {
	Geo32 r;
	r.slab = g.nd - 1;
	int s = 1;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		r.T[d] = (d == r.slab) ? g.nloc : g.T[d];
		r.stride[d] = s;
		if (d < g.nd) s *= (d == r.slab) ? (g.nloc + 2) : r.T[d];
	}
	return r;
}
// (node coordinates and strides are < 2^24: 24-bit multiplies, full rate)
__device__ __forceinline__ int mul24(int a, int b) { return (int)__umul24((unsigned)a, (unsigned)b); }
__device__ __forceinline__ void node_pair(const Geo32 &G, int d, int j, int &o0, int &o1) {
	if (d == G.slab) {
		o0 = d ? mul24(j, G.stride[d]) : j;
		o1 = o0 + G.stride[d];
	} else {
		// wrap_pad of j and j+1 (padded coordinates 0..T+1; a periodic image
		// of the block's boxes may lie one period either side, -T < j < 2T)
		int s0 = j - 1, s1 = j;
		s0 = s0 < 0 ? s0 + G.T[d] : (s0 >= G.T[d] ? s0 - G.T[d] : s0);
		s1 = s1 < 0 ? s1 + G.T[d] : (s1 >= G.T[d] ? s1 - G.T[d] : s1);
		o0 = d ? mul24(s0, G.stride[d]) : s0;
		o1 = d ? mul24(s1, G.stride[d]) : s1;
	}
}
// periodic images of the cells nearest to the block's reference cell r (the
// cell of its first item).  The half cells 0 and T (thresholds at 0.5 and
// T + 0.5) are one cell of the torus: a particle that crosses T + 0.5 lands
// in cell 0 while its neighbours stay in cell T, and the block's boxes,
// centred on the mean cell, would sit between the two.  E at image nodes is
// the same data (wrapped storage; the slab's ghost planes when the slab
// dimension wraps, whose images stay within cells 0..T).  Block-uniform
// bounds: cells <= lo move up by T, cells >= hi down by T.
struct Images {
	int lo[3], hi[3], T[3];
	__device__ __forceinline__ int operator()(int d, int c) const {
		return c + (c <= lo[d] ? T[d] : 0) - (c >= hi[d] ? T[d] : 0);
	}
};
__device__ __forceinline__ Images make_images(const Geo32 &G, int wrapMask, const int *r, int nd) {
	Images m;
	for (int d = 0; d < 3; d++) {
		const int T = G.T[d], h = T / 2;
		m.T[d] = T;
		m.lo[d] = INT32_MIN;
		m.hi[d] = INT32_MAX;
		if (d >= nd) continue;
		if (d != G.slab) {
			m.lo[d] = r[d] - h - 1;
			m.hi[d] = r[d] + h + 1;
		} else if ((wrapMask >> d) & 1) {
			m.lo[d] = min(r[d] - h - 1, 0);
			m.hi[d] = max(r[d] + h + 1, T);
		}
	}
	return m;
}

// LDS capacities of the push: E nodes (pre-move cells + 1), charge nodes
// (post-move cells + 1), input cells and output cells of the sort counters
// (the sorting push, whose LDS also holds the rank array, keeps the smaller
// charge box).  The unsorted push's boxes take a chunk that straddles
// two tiles (8 x 4 x 4 cells) after a step of motion ((10 x 6 x 6 cells):
// 539 E nodes, 1053 charge nodes); with 384 and 1024 such chunks -- a
// quarter of them -- gathered E and added charge through global memory.
constexpr int kRhoBoxCap = 1024;
constexpr int kEBoxCapPlain = 768;
constexpr int kEBoxCapSort = 768;
constexpr int kInCellCap = 256;
constexpr int kOutCellCap = 512;

// box of integer coordinates: origin, extents, volume, linear index
struct Box {
	int lo[3], n[3];
	int vol;
	__device__ __forceinline__ int index(const int *c, int nd) const {
		int l = 0, s = 1;
		for (int d = 0; d < nd; d++) {
			l += mul24(c[d] - lo[d], s);
			s *= n[d];
		}
		return l;
	}
	__device__ __forceinline__ bool inside(const int *c, int nd) const {
		bool ok = vol > 0;
		for (int d = 0; d < nd; d++) ok = ok && c[d] >= lo[d] && c[d] < lo[d] + n[d];
		return ok;
	}
};
// Box coordinates of linear index l < vol without integer division: the
// block-uniform reciprocals of the extents (box_rcp) and one float multiply
// per dimension.  (l + 0.5) / n lies at least 0.5 / n from an integer and
// the float product errs by less than 2^-12 for l < 2^11 (the boxes hold at
// most 2048 nodes, extents <= 2 kBoxReach + 4), so the quotient is exact.
struct BoxRcp {
	float r[3];
};
__device__ __forceinline__ BoxRcp box_rcp(const Box &b) {
	BoxRcp q;
#pragma unroll
	for (int d = 0; d < 3; d++) q.r[d] = 1.0f / (float)b.n[d];
	return q;
}
__device__ __forceinline__ void box_coords(const Box &b, const BoxRcp &q, int l, int *c, int nd) {
#pragma unroll
	for (int d = 0; d < 3; d++) {
		if (d >= nd) break;
		if (d == nd - 1) {
			c[d] = b.lo[d] + l;
			break;
		}
		const int qd = (int)(((float)l + 0.5f) * q.r[d]);
		c[d] = b.lo[d] + (l - qd * b.n[d]);
		l = qd;
	}
}
// Box of the cells clo..chi grown by grow_lo/grow_hi, trimmed to at most cap
// entries: each dimension first to kBoxReach cells either side of the mean
// cell mid, then the widest one cell at a time from its side farther from mid
// (block-uniform; vol 0 if even a single cell does not fit).
constexpr int kBoxReach = 8;
__device__ __forceinline__ Box make_box(const int *clo, const int *chi, const int *mid, int grow_lo, int grow_hi,
                                        int nd, int cap) {
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
	for (int d = 0; d < nd; d++) {
		lo[d] = max(clo[d], mid[d] - kBoxReach);
		hi[d] = min(chi[d], mid[d] + kBoxReach);
		if (lo[d] > hi[d]) lo[d] = hi[d] = mid[d];
	}
	long v = 0;
#pragma unroll 1
	for (int it = 0; it < 6 * kBoxReach + 3; it++) {
		v = 1;
		int w = 0;
		for (int d = 0; d < nd; d++) {
			v *= hi[d] - lo[d] + 1 + grow_lo + grow_hi;
			if (hi[d] - lo[d] > hi[w] - lo[w]) w = d;
		}
		if (v <= cap || hi[w] == lo[w]) break;
		if (hi[w] - mid[w] >= mid[w] - lo[w]) hi[w]--;
		else lo[w]++;
	}
	Box b;
	for (int d = 0; d < 3; d++) {
		b.lo[d] = d < nd ? lo[d] - grow_lo : 0;
		b.n[d] = d < nd ? hi[d] - lo[d] + 1 + grow_lo + grow_hi : 1;
	}
	b.vol = (v <= cap && v > 0) ? (int)v : 0;
	return b;
}

// sort key of integer cell coordinates (tile_key's order)
template <int ND>
__device__ __forceinline__ int tile_key_cells(const TileGeo &tg, const int *cin) {
	int c[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) c[d] = cin[d] < 0 ? 0 : (cin[d] > tg.cmax[d] ? tg.cmax[d] : cin[d]);
	return tile_key_of<ND>(tg, c);
}

// Bricks (TileGeo::bs) of a cell box: brick coordinates = clamped cell >> bs.
// A brick's cells have consecutive keys, so the sorting push reserves one
// range per brick and block from the cursor of the brick's first cell (the
// counts and the scan stay per cell; the other cells' cursors go unused).
struct BrickBox {
	int lo[3], n[3];
	int vol;
};
template <int ND>
__device__ __forceinline__ int clamp_cell(const TileGeo &tg, int d, int c) {
	return c < 0 ? 0 : (c > tg.cmax[d] ? tg.cmax[d] : c);
}
// brick box of a cell box (at most as many entries as the cell box)
template <int ND>
__device__ __forceinline__ BrickBox make_brick_box(const TileGeo &tg, const Box &b) {
	BrickBox r;
	r.vol = b.vol > 0 ? 1 : 0;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		r.lo[d] = d < ND ? clamp_cell<ND>(tg, d, b.lo[d]) >> tg.bs[d] : 0;
		r.n[d] = d < ND ? (clamp_cell<ND>(tg, d, b.lo[d] + b.n[d] - 1) >> tg.bs[d]) - r.lo[d] + 1 : 1;
		r.vol *= r.n[d];
	}
	return r;
}
// Brick box of the cells within `reach` of the block's mean cell (clipped to
// its extent clo..chi), trimmed to at most cap bricks -- the widest dimension
// first, from its side farther from the mean -- but never inside `core`.
template <int ND>
__device__ __forceinline__ BrickBox wide_brick_box(const TileGeo &tg, const int *clo, const int *chi, const int *mid,
                                                   int reach, int cap, const BrickBox &core) {
	int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, m[3] = {0, 0, 0}, flo[3] = {0, 0, 0}, fhi[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		int l = max(clo[d], mid[d] - reach), h = min(chi[d], mid[d] + reach);
		if (l > h) l = h = mid[d];
		m[d] = clamp_cell<ND>(tg, d, mid[d]) >> tg.bs[d];
		flo[d] = core.vol ? core.lo[d] : m[d];
		fhi[d] = core.vol ? core.lo[d] + core.n[d] - 1 : m[d];
		lo[d] = min(clamp_cell<ND>(tg, d, l) >> tg.bs[d], flo[d]);
		hi[d] = max(clamp_cell<ND>(tg, d, h) >> tg.bs[d], fhi[d]);
	}
	int v = 0;
#pragma unroll 1
	for (int it = 0; it < 128; it++) {
		v = 1;
		for (int d = 0; d < ND; d++) v *= hi[d] - lo[d] + 1;
		if (v <= cap) break;
		int w = -1;
		for (int d = 0; d < ND; d++)
			if ((lo[d] < flo[d] || hi[d] > fhi[d]) && (w < 0 || hi[d] - lo[d] > hi[w] - lo[w])) w = d;
		if (w < 0) break;
		if (hi[w] > fhi[w] && (lo[w] >= flo[w] || hi[w] - m[w] >= m[w] - lo[w])) hi[w]--;
		else lo[w]++;
	}
	// block-uniform: scalar registers
	BrickBox b;
#pragma unroll
	for (int d = 0; d < 3; d++) {
		b.lo[d] = __builtin_amdgcn_readfirstlane(lo[d]);
		b.n[d] = __builtin_amdgcn_readfirstlane(hi[d] - lo[d] + 1);
	}
	b.vol = __builtin_amdgcn_readfirstlane(v <= cap ? v : 0);
	return b;
}
// index in the brick box of the brick holding cell c, or -1 outside it
template <int ND>
__device__ __forceinline__ int brick_inside(const TileGeo &tg, const BrickBox &bb, const int *c) {
	int l = 0, s = 1;
	bool in = bb.vol > 0;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		const int r = (clamp_cell<ND>(tg, d, c[d]) >> tg.bs[d]) - bb.lo[d];
		in &= (unsigned)r < (unsigned)bb.n[d];
		l += mul24(r, s);
		s *= bb.n[d];
	}
	return in ? l : -1;
}
// key of the first cell of the brick holding cell c
template <int ND>
__device__ __forceinline__ int brick_first_key(const TileGeo &tg, const int *c) {
	int f[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) f[d] = (clamp_cell<ND>(tg, d, c[d]) >> tg.bs[d]) << tg.bs[d];
	return tile_key_cells<ND>(tg, f);
}
// key of the first cell of brick l of a brick box
template <int ND>
__device__ __forceinline__ int brick_key(const TileGeo &tg, const BrickBox &bb, int l) {
	int c[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		c[d] = (bb.lo[d] + l % bb.n[d]) << tg.bs[d];
		l /= bb.n[d];
	}
	return tile_key_cells<ND>(tg, c);
}

typedef double dvec2 __attribute__((ext_vector_type(2)));

// chunk of push block b of nb: consecutive chunks (the same cell tiles after
// a sort: shared E nodes and rho atomics) on one XCD's L2.
// Blocks are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md,
// workgroup dispatch), so block b runs on XCD b % 8; the map is a bijection
// for any grid size and only a placement hint, never needed for
// correctness.  (Host and device: the push trace attributes chunks to XCDs
// with it, pinc_hip_push_xcd_of_chunk.)
__host__ __device__ __forceinline__ unsigned push_chunk_of(unsigned nb, unsigned b) {
	// pieces of kPushXcdPiece consecutive chunks dealt round-robin over
	// the XCDs (the tail beyond whole rounds in order): every XCD gets pieces
	// from every part of the array, e.g. both z faces' tiles, where wrapped
	// particles make blocks slower (C4: step 55.39 -> 55.07 ms against
	// contiguous eighths, which left the XCD holding the top z tiles 1.2 ms
	// behind the others on the electrons)
	constexpr unsigned P = kPushXcdPiece;
	const unsigned F = nb / (8u * P) * (8u * P);
	if (b >= F) return b;
	const unsigned x = b & 7u, y = b >> 3;
	return ((y / P) * 8u + x) * P + (y % P);
}

// OBJ: the object test of the fused collection (separate instances, so the
// plain push carries none of its code)
template <int ND, bool V3D, bool KICK, bool SORT, bool OBJ = false>
__global__ __launch_bounds__(kPushThreads) __attribute__((amdgpu_waves_per_eu(kPushWavesPerEu))) void k_push(PushArgs a) {
	constexpr int NC = 1 << ND;
	constexpr int NW = kPushThreads / 64;
	// the sorting push keeps its LDS at 40 KB (4 blocks per CU): fewer copies
	constexpr int RL = SORT ? 1024 : kRhoLds;
	__shared__ double rhoL[RL];
	// staged E box: 3-D (E_x, E_y) pairs at eL[2t] (one ds_read_b128 per
	// corner) and E_z at eL[2 cap + t], else value-major
	constexpr int EC = SORT ? kEBoxCapSort : kEBoxCapPlain;  // E box capacity (nodes)
	constexpr int RC = SORT ? kRhoBoxCap : RL;              // charge box capacity (nodes)
	constexpr int kEL = KICK ? EC * ND : 1;
	__shared__ __attribute__((aligned(16))) double eLs[kEL];
	double *const eL = eLs;
	__shared__ int cntOut[kOutCellCap];
	__shared__ int red[3 * 3 * NW];
	__shared__ int cbox[9];
	__shared__ double kered[NW];
	__shared__ int wcnt[NW];
	__shared__ int wmov[NW];
	// sorting push, per item: its rank code (phase C) and its flag (phase D)
	__shared__ int rlL[SORT ? kPushChunk : 1];
	// sorting push: counters, then exclusive offsets, of (brick, cell in brick)
	__shared__ int ccL[SORT ? kCellRankBricks * 16 : 1];
	__shared__ unsigned char stageF[SORT ? kPushChunk : 1];
	const Geo32 G = make_geo32(a.g);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	// chunk of this block (push_chunk_of: XCD-aware placement)
	const unsigned chunk = push_chunk_of(gridDim.x, blockIdx.x);
	const long base = (long)chunk * kPushChunk;
	// item k of a thread: the kPushItems particles of a thread are
	// consecutive, so a thread's particles mostly share a cell and their
	// charge is summed in the thread before the LDS adds; rows of 16 lanes swap
	// halves so that full blocks load and store contiguously: row r of a wave
	// holds the 64 consecutive particles at {0, 128, 64, 192}[r], lane i of it
	// those at 4i of them
	static_assert(kPushItems == 4 && kPushThreads % 64 == 0, "lane exchange: four items per thread");
	auto item = [&](int k) -> long {
		return base + (long)(wv * 256 + ((lane >> 4) & 1) * 128 + (lane >> 5) * 64 + (lane & 15) * 4 + k);
	};
	// pairs are 16-B aligned when every species array is (the species
	// offset iStart is even); otherwise one 8-B access per particle
	bool al = true;
#pragma unroll
	for (int d = 0; d < ND; d++)
		al = al && !((reinterpret_cast<unsigned long>(a.xi[d]) | reinterpret_cast<unsigned long>(a.vi[d]) |
		              reinterpret_cast<unsigned long>(a.xo[d]) | reinterpret_cast<unsigned long>(a.vo[d])) & 15);

	unsigned long long tsub = 0;  // (trace mode: thread 0's last timestamp)
	PUSH_TS(0);
	// ---- phase A: load every item, cell box of the input positions (periodic
	// images nearest to the cell of the block's first item)
	// (loaded first, converted after the item loads are issued: the oldest
	// load in flight, so its wait does not hold back the items')
	double xref[3] = {1.0, 1.0, 1.0};
	if (base < a.n) {
#pragma unroll
		for (int d = 0; d < ND; d++) xref[d] = a.xi[d][base];
	}
	double p[kPushItems][ND], vv[kPushItems][ND];
	unsigned valid = 0;
	static_assert(kPushItems % 2 == 0, "items come in pairs");
	// a full block of aligned arrays: two contiguous 16-B loads per array and
	// thread
	const bool full = al && base + kPushChunk <= a.n;
	// lane l loads pair pi(l) and 64 + pi(l) of the wave's 128: rows 0
	// and 1 (2 and 3) interleave pairs 0..31 (32..63) even/odd, so the row
	// swap (v_permlane16_swap: odd rows of the first <-> even rows of the
	// second) leaves each lane two consecutive pairs; every wave instruction
	// still covers one contiguous 1 KB
	auto pi_lane = [](int l) { return ((l >> 5) << 5) + 2 * (l & 15) + ((l >> 4) & 1); };
	auto rowswap = [](dvec2 &u, dvec2 &w) {
		typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
		u32x4 A = __builtin_bit_cast(u32x4, u), B = __builtin_bit_cast(u32x4, w);
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const auto r = __builtin_amdgcn_permlane16_swap(A[i], B[i], false, false);
			A[i] = r[0];
			B[i] = r[1];
		}
		u = __builtin_bit_cast(dvec2, A);
		w = __builtin_bit_cast(dvec2, B);
	};
	if (full) {
		valid = (1u << kPushItems) - 1;
		const long q0 = base + wv * 256 + 2 * pi_lane(lane);
		auto ld = [](const double *ptr) -> dvec2 {
			return __builtin_nontemporal_load(reinterpret_cast<const dvec2 *>(ptr));
		};
#pragma unroll
		for (int d = 0; d < ND; d++) {
			dvec2 x0 = ld(a.xi[d] + q0);
			dvec2 x1 = ld(a.xi[d] + q0 + 128);
			dvec2 v0 = ld(a.vi[d] + q0);
			dvec2 v1 = ld(a.vi[d] + q0 + 128);
			rowswap(x0, x1);
			rowswap(v0, v1);
			p[0][d] = x0.x;
			p[1][d] = x0.y;
			p[2][d] = x1.x;
			p[3][d] = x1.y;
			vv[0][d] = v0.x;
			vv[1][d] = v0.y;
			vv[2][d] = v1.x;
			vv[3][d] = v1.y;
		}
	} else
#pragma unroll
	for (int k = 0; k < kPushItems; k += 2) {
		const long i = item(k);
		const bool ok0 = i < a.n, ok1 = i + 1 < a.n;
		valid |= ((unsigned)ok0 | (unsigned)ok1 << 1) << k;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			if (ok1 && al) {
				const dvec2 x = *reinterpret_cast<const dvec2 *>(a.xi[d] + i);
				const dvec2 v = *reinterpret_cast<const dvec2 *>(a.vi[d] + i);
				p[k][d] = x.x;
				p[k + 1][d] = x.y;
				vv[k][d] = v.x;
				vv[k + 1][d] = v.y;
			} else {
				p[k][d] = ok0 ? a.xi[d][i] : 1.0;
				vv[k][d] = ok0 ? a.vi[d][i] : 0.0;
				p[k + 1][d] = ok1 ? a.xi[d][i + 1] : 1.0;
				vv[k + 1][d] = ok1 ? a.vi[d][i + 1] : 0.0;
			}
		}
	}
	int cref[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) cref[d] = __builtin_amdgcn_readfirstlane((int)xref[d]);
	// main.c's double fold (literal loop): a deposit on a slab ghost plane
	// counts twice and literal_ghost_weights adds that weight at the cell's
	// own planes, so the slab dimension keeps its unmapped cells there (an
	// image would move weight between ghost plane 0 and true plane T, which
	// one fold treats alike and two do not)
	const int imgMask = a.g.literal ? (a.wrapMask & ~(1 << G.slab)) : a.wrapMask;
	const Images img = make_images(G, imgMask, cref, ND);
	// cell range (and sum) of the block's items, in raw cells or in the
	// images nearest the reference cell
	auto cell_box = [&](bool withImg) {
		int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN}, sm[3] = {0, 0, 0};
#pragma unroll
		for (int k = 0; k < kPushItems; k += 2) {
#pragma unroll
			for (int d = 0; d < ND; d++) {
#pragma unroll
				for (int h = 0; h < 2; h++) {
					if ((valid >> (k + h)) & 1u) {
						const int c = withImg ? img(d, (int)p[k + h][d]) : (int)p[k + h][d];
						lo[d] = min(lo[d], c);
						hi[d] = max(hi[d], c);
						sm[d] += c;
					}
				}
			}
		}
#pragma unroll
		for (int d = 0; d < ND; d++) {
			int x = wave_min_i(lo[d]), y = wave_max_i(hi[d]), z = wave_sum_i(sm[d]);
			if (lane == 0) {
				red[(3 * d) * NW + wv] = x;
				red[(3 * d + 1) * NW + wv] = y;
				red[(3 * d + 2) * NW + wv] = z;
			}
		}
		__syncthreads();
		if (threadIdx.x < ND) {
			int d = threadIdx.x, x = INT32_MAX, y = INT32_MIN, z = 0;
			for (int w = 0; w < NW; w++) {
				x = min(x, red[(3 * d) * NW + w]);
				y = max(y, red[(3 * d + 1) * NW + w]);
				z += red[(3 * d + 2) * NW + w];
			}
			const int nv = (int)min((long)kPushChunk, a.n - base);
			cbox[d] = x;
			cbox[3 + d] = y;
			cbox[6 + d] = nv > 0 ? z / nv : 0;
		}
		__syncthreads();
	};
	// The images differ from the raw cells only for a block whose items
	// straddle a periodic boundary: with every raw cell within T/2 - 2 of the
	// reference cell, the pre-move cells and the post-move cells of the
	// particles that stay in place (one cell of motion) all lie strictly
	// between the images' bounds, so img() is the identity there.  Such
	// blocks (nearly all) skip the per-item image arithmetic in the box, the
	// kick and the deposit; a particle that wrapped in place lands outside
	// the charge box and adds its weights through memory (the same nodes, a
	// different summation order).  The others take the raw box first, then
	// the images' box.
	cell_box(false);
	bool useImg = false;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		const int x = __builtin_amdgcn_readfirstlane(cbox[d]), y = __builtin_amdgcn_readfirstlane(cbox[3 + d]);
		useImg |= x <= y && (img.lo[d] != INT32_MIN || img.hi[d] != INT32_MAX) &&
		          (cref[d] - x > G.T[d] / 2 - 2 || y - cref[d] > G.T[d] / 2 - 2);
	}
	if (useImg) cell_box(true);
	int clo[3] = {0, 0, 0}, chi[3] = {0, 0, 0}, cmid[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		// block-uniform: scalar registers, so the boxes cost no VGPRs
		clo[d] = __builtin_amdgcn_readfirstlane(cbox[d]);
		chi[d] = __builtin_amdgcn_readfirstlane(cbox[3 + d]);
		cmid[d] = __builtin_amdgcn_readfirstlane(cbox[6 + d]);
	}
	const bool empty = clo[0] > chi[0];
	// E nodes of the input cells; charge nodes and cells after a move of at
	// most one cell (|v| <= maxVel <= 1).  Each box is trimmed around the
	// block's mean cell to its LDS capacity; the items outside it (far movers,
	// wrapped particles) take the global path.
	const Box eB = (KICK && !empty) ? make_box(clo, chi, cmid, 0, 1, ND, EC) : Box{{0, 0, 0}, {1, 1, 1}, 0};
	const Box rB = !empty ? make_box(clo, chi, cmid, 1, 2, ND, RC) : Box{{0, 0, 0}, {1, 1, 1}, 0};
	// (the sorting push's cell box: the core of its brick box ib below)
	const int ahead = 1;  // (sort cells: input cells +-1, sort_cell)
	const Box iB = (SORT && !empty) ? make_box(clo, chi, cmid, ahead, ahead, ND, kInCellCap) : Box{{0, 0, 0}, {1, 1, 1}, 0};
	// the sorting push reserves per brick from the cursor of the brick's
	// first cell, so the counting push counts per brick (at its first key):
	// a block's output falls into a few bricks.  Only the brick counters live
	// in LDS, so the cell box they cover may be 16 times their number; a
	// brick box beyond the counters (far movers) counts in memory.
	const Box oB = (a.cntNext && !empty) ? make_box(clo, chi, cmid, 1 + ahead, 1 + ahead, ND, 16 * kOutCellCap)
	                                     : Box{{0, 0, 0}, {1, 1, 1}, 0};
	BrickBox obb = (a.cntNext && !empty) ? make_brick_box<ND>(a.tg, oB) : BrickBox{{0, 0, 0}, {1, 1, 1}, 0};
	if (obb.vol > kOutCellCap) obb.vol = 0;
	// sorting push: the items inside the wide brick box ib are ranked by
	// brick (one run of each brick per block); only items outside it take a
	// global slot one by one.  The brick counters live in cntOut, which a
	// sorting push does not use (it never counts).
	int slo[3] = {0, 0, 0}, shi[3] = {0, 0, 0};
#pragma unroll
	for (int d = 0; d < ND; d++) {
		slo[d] = clo[d] - ahead;
		shi[d] = chi[d] + ahead;
	}
	const BrickBox ib = (SORT && !empty)
	                        ? wide_brick_box<ND>(a.tg, slo, shi, cmid, 8, kInCellCap, make_brick_box<ND>(a.tg, iB))
	                        : BrickBox{{0, 0, 0}, {1, 1, 1}, 0};
	static_assert(kOutCellCap >= 2 * kInCellCap, "brick counters in cntOut");
	int *const bCnt = cntOut, *const bBase = cntOut + kInCellCap;

	PUSH_TS(1);
	// ---- phase B: LDS setup (zero the accumulators, stage E)
	// copies of the charge box (at most kPushCopies): odd stride, so that the
	// copies of a node fall in different LDS banks
	const int rStride = rB.vol | 1;
	int nCopy = 1;
	while (nCopy < kPushCopies && 2 * nCopy * rStride <= RL) nCopy *= 2;
	const int myCopy = (lane & (nCopy - 1)) * rStride;
	for (int t = threadIdx.x; t < nCopy * rStride; t += kPushThreads) rhoL[t] = 0.0;
	for (int t = threadIdx.x; t < (SORT ? kInCellCap : obb.vol); t += kPushThreads) cntOut[t] = 0;
	// (cell ranking: block-uniform; bricks of at most 16 cells)
	const int brickCellBits = a.tg.bs[0] + a.tg.bs[1] + a.tg.bs[2];
	const bool cellRank = SORT && ib.vol <= kCellRankBricks && brickCellBits <= 4;
	if (cellRank)
		for (int t = threadIdx.x; t < ib.vol * 16; t += kPushThreads) ccL[t] = 0;
	if (KICK) {
		const BoxRcp eq = box_rcp(eB);
		for (int t = threadIdx.x; t < eB.vol; t += kPushThreads) {
			int c[3] = {0, 0, 0};
			box_coords(eB, eq, t, c, ND);
			int off = 0;
#pragma unroll
			for (int d = 0; d < ND; d++) {
				int o0, o1;
				node_pair(G, d, c[d], o0, o1);
				off += o0;
			}
			const double *ep = a.Es + (unsigned)(off * ND);
			if constexpr (ND == 3) {
				eL[2 * t] = ep[0];
				eL[2 * t + 1] = ep[1];
				eL[2 * EC + t] = ep[2];
			} else {
#pragma unroll
				for (int q = 0; q < ND; q++) eL[t * ND + q] = ep[q];
			}
		}
	}
	__syncthreads();

	int resBase = 0;  // sorting push: this thread's brick reservation
	PUSH_TS(2);
	// ---- phase C (sorted output): rank of every item inside its brick's run,
	// and one global reservation per brick of the block.  Per item, in LDS
	// (the sort push is tight on VGPRs): rank << 8 | brick of ib, or ~global
	// slot for an item outside ib.  A brick's run holds its cells in the order
	// the items reach the counter: a wave instruction's same-cell lanes stay
	// together, so a thread's consecutive output particles mostly share a cell
	// (round 4: ranking by cell inside each brick first cost a pass and two
	// barriers; C4 electron sorting push 33.9 -> 32.0 ms, the plain pushes
	// after it +1 %).
	if (SORT) {
		static_assert(kInCellCap <= 256 && kPushChunk <= (1 << 23), "rank/brick packing");
		static_assert(kCellRankBricks <= 64 && kPushChunk <= (1 << 20), "rank/brick/cell packing");
		int no = 0;  // (trace: items outside ib)
#pragma unroll
		for (int k = 0; k < kPushItems; k++) {
			int c[3] = {0, 0, 0};
#pragma unroll
			for (int d = 0; d < ND; d++) c[d] = sort_cell(p[k][d], vv[k][d]);
			const bool ok = (valid >> k) & 1u;
			const int lb = ok ? brick_inside<ND>(a.tg, ib, c) : -1;
			// plain LDS atomics: a wave's lanes share a few bricks (same-address
			// conflicts), cheaper than aggregating the groups with ballots and
			// shuffles (C4 electron sorting push 36.2 -> 33.5 ms)
			int rank = 0, rl = -1;
			if (cellRank) {
				// the cell's index inside its brick, x fastest (clamped as brick_inside)
				int ci = 0, sh = 0;
#pragma unroll
				for (int d = 0; d < ND; d++) {
					ci |= (clamp_cell<ND>(a.tg, d, c[d]) & ((1 << a.tg.bs[d]) - 1)) << sh;
					sh += a.tg.bs[d];
				}
				rank = lb >= 0 ? atomicAdd(&ccL[lb * 16 + ci], 1) : 0;
				rl = rank << 10 | lb << 4 | ci;
			} else {
				rank = lb >= 0 ? atomicAdd(&bCnt[lb], 1) : 0;
				rl = rank << 8 | lb;
			}
			const bool out = ok && lb < 0;
			const int g = agg_add(a.cursor, out ? brick_first_key<ND>(a.tg, c) : 0, out);
			rl = lb >= 0 ? rl : (ok ? ~g : -1);
			rlL[k * kPushThreads + threadIdx.x] = rl;  // (stored at once: no item's rank stays live)
			no += rl < 0 && ok;
		}
		if (a.diag) {
			no = wave_sum_i(no);
			if (lane == 0 && no) atomicAdd(&a.diag[0], (unsigned long long)no);
		}
		__syncthreads();
		PUSH_SUB(4);
		static_assert(kInCellCap <= kPushThreads, "one reservation per thread");
		// one global reservation per brick of ib, one range of its first
		// cell's cursor
		int bm = 0;
		if (cellRank) {
			// each brick's cell counters to exclusive offsets inside its run
			if ((int)threadIdx.x < ib.vol) {
#pragma unroll
				for (int q = 0; q < 16; q++) {
					const int v = ccL[threadIdx.x * 16 + q];
					ccL[threadIdx.x * 16 + q] = bm;
					bm += v;
				}
			}
		} else {
			bm = (int)threadIdx.x < ib.vol ? bCnt[threadIdx.x] : 0;
		}
		// the global reservation's result is first needed by the stores after
		// the kick: its round trip overlaps the kick (resBase, one VGPR)
		if (bm) resBase = atomicAdd(&a.cursor[brick_key<ND>(a.tg, ib, threadIdx.x)], bm);
	}

	PUSH_TS(3);
	// ---- phase D: kick, drift, classify (unsorted: store)
	// value offsets of the 2^ND corners in the staged E box (block-uniform)
	int eoffs[NC];
#pragma unroll
	for (int c = 0; c < NC; c++) {
		int o = 0, st = 1;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			o += ((c >> d) & 1) ? st : 0;
			st *= eB.n[d];
		}
		eoffs[c] = ND == 3 ? o : o * ND;
	}
	double ke = 0.0;
	int cnt = 0, bad = 0;
	unsigned dep = 0;
	bool thrInFrame = true;
#pragma unroll
	for (int d = 0; d < ND; d++) thrInFrame &= a.thr.lo[d] >= 0.0 && a.thr.up[d] <= a.thr.hi[d];
	// positions (and velocities if kicked or moved) of items k, k + 1
	const bool wvel = KICK || a.vo[0] != a.vi[0];
	auto store_pair = [&](int k) {
		const long i = item(k);
		const bool ok0 = (valid >> k) & 1u, ok1 = (valid >> (k + 1)) & 1u;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			if (ok1 && al) {
				*reinterpret_cast<dvec2 *>(a.xo[d] + i) = dvec2{p[k][d], p[k + 1][d]};
				if (wvel) *reinterpret_cast<dvec2 *>(a.vo[d] + i) = dvec2{vv[k][d], vv[k + 1][d]};
			} else {
				if (ok0) a.xo[d][i] = p[k][d];
				if (ok0 && wvel) a.vo[d][i] = vv[k][d];
				if (ok1) a.xo[d][i + 1] = p[k + 1][d];
				if (ok1 && wvel) a.vo[d][i + 1] = vv[k + 1][d];
			}
		}
	};
#pragma unroll
	for (int k = 0; k < kPushItems; k++) {
		if (!((valid >> k) & 1u)) continue;
		const long i = item(k);
		if (KICK) {
			double dec[3], comp[3];
			int j[3] = {0, 0, 0}, jc[3] = {0, 0, 0};
#pragma unroll
			for (int d = 0; d < ND; d++) {
				j[d] = (int)p[k][d];
				jc[d] = j[d];
				dec[d] = p[k][d] - j[d];
				comp[d] = 1 - dec[d];
			}
			if (useImg) {
#pragma unroll
				for (int d = 0; d < ND; d++) jc[d] = img(d, j[d]);
			}
			// all 2^ND corners in the staged box: one unsigned compare per
			// dimension, evaluated without short-circuit branches
			bool inE = eB.vol > 0;
#pragma unroll
			for (int d = 0; d < ND; d++) inE &= (unsigned)(jc[d] - eB.lo[d]) < (unsigned)(eB.n[d] - 1);
			if (a.diag) {  // (trace: [1] += particles that gather E from memory, [3] += those of them
				           // more than a quarter of the grid from the box: periodic wraps)
				const int ng = __popcll(__ballot(!inE));
				bool far = false;
#pragma unroll
				for (int d = 0; d < ND; d++) far |= abs(jc[d] - (eB.lo[d] + eB.n[d] / 2)) > G.T[d] / 4;
				const int nf = __popcll(__ballot(!inE && far));
				if (lane == 0 && ng) atomicAdd(&a.diag[1], (unsigned long long)ng);
				if (lane == 0 && nf) atomicAdd(&a.diag[3], (unsigned long long)nf);
			}
			double dv[ND];
			if constexpr (V3D) {
				// puInterp3D1 (pusher.c:1116-1120), corner c = x + 2y + 4z, one
				// component at a time (E_x and E_y from one 16-B LDS read per
				// corner, then E_z): 16 corner values live instead of 24
				const double x = dec[0], y = dec[1], z = dec[2];
				const double xc = comp[0], yc = comp[1], zc = comp[2];
				auto interp = [&](const double *f) -> double {
					return zc * (yc * (xc * f[0] + x * f[1]) + y * (xc * f[2] + x * f[3])) +
					       z * (yc * (xc * f[4] + x * f[5]) + y * (xc * f[6] + x * f[7]));
				};
				if (inE) {
					const int ei = eB.index(jc, ND);
					double fx[NC], fy[NC];
#pragma unroll
					for (int c = 0; c < NC; c++) {
						const dvec2 xy = *reinterpret_cast<const dvec2 *>(eL + 2 * (ei + eoffs[c]));
						fx[c] = xy.x;
						fy[c] = xy.y;
					}
					dv[0] = interp(fx);
					dv[1] = interp(fy);
					__builtin_amdgcn_sched_barrier(0);
					double fz[NC];
#pragma unroll
					for (int c = 0; c < NC; c++) fz[c] = eL[2 * EC + ei + eoffs[c]];
					dv[2] = interp(fz);
				} else {
					int o[3][2];
#pragma unroll
					for (int d = 0; d < ND; d++) node_pair(G, d, j[d], o[d][0], o[d][1]);
					unsigned off[NC];
#pragma unroll
					for (int c = 0; c < NC; c++) {
						int t = 0;
#pragma unroll
						for (int d = 0; d < ND; d++) t += o[d][(c >> d) & 1];
						off[c] = (unsigned)(t * ND);
					}
#pragma unroll
					for (int q = 0; q < ND; q++) {
						double f[NC];
#pragma unroll
						for (int c = 0; c < NC; c++) f[c] = a.Es[off[c] + q];
						dv[q] = interp(f);
					}
				}
			} else {
				double e[NC][ND];
				if (inE) {
					const double *eb = eL + mul24(eB.index(jc, ND), ND);
#pragma unroll
					for (int c = 0; c < NC; c++)
#pragma unroll
						for (int q = 0; q < ND; q++) e[c][q] = eb[eoffs[c] + q];
				} else {
					int o[3][2];
#pragma unroll
					for (int d = 0; d < ND; d++) node_pair(G, d, j[d], o[d][0], o[d][1]);
#pragma unroll
					for (int c = 0; c < NC; c++) {
						int off = 0;
#pragma unroll
						for (int d = 0; d < ND; d++) off += o[d][(c >> d) & 1];
						const double *ep = a.Es + (unsigned)(off * ND);
#pragma unroll
						for (int q = 0; q < ND; q++) e[c][q] = ep[q];
					}
				}
				// puInterpND1Inner: corner by corner in the recursion order
#pragma unroll
				for (int q = 0; q < ND; q++) dv[q] = 0;
#pragma unroll
				for (int c = 0; c < (1 << (ND - 1)); c++) {
					double f = 1.0;
					int cc = 0;
#pragma unroll
					for (int d = ND - 1; d >= 1; d--) {
						int bit = (c >> (d - 1)) & 1;
						f = (bit ? dec[d] : comp[d]) * f;
						cc |= bit << d;
					}
#pragma unroll
					for (int q = 0; q < ND; q++) {
						dv[q] += comp[0] * f * e[cc][q];
						dv[q] += dec[0] * f * e[cc | 1][q];
					}
				}
			}
			double vsq = 0;
#pragma unroll
			for (int d = 0; d < ND; d++) {
				vsq += vv[k][d] * (vv[k][d] + dv[d]);
				vv[k][d] = vv[k][d] + dv[d];
			}
			ke += vsq;
		}
		// drift + pVelAssertMax (population.c:342-365)
		int chg = 0;
		int c0[3] = {0, 0, 0};  // pre-move cell (the statistic below)
#pragma unroll
		for (int d = 0; d < ND; d++) c0[d] = (int)p[k][d];
#pragma unroll
		for (int d = 0; d < ND; d++) {
			bad |= (vv[k][d] > a.maxVel);
			p[k][d] += vv[k][d];
			// cell changed (statistic for the sort schedule; recomputed, not kept)
			chg |= (int)p[k][d] != c0[d];
		}
		// neighbour digit per dimension, as k_move_classify
		int ne = 0;
		bool outside = false;
		int digs[3] = {1, 1, 1};
		bool leaves = false;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			digs[d] = 1 - (p[k][d] < a.thr.lo[d]) + (p[k][d] >= a.thr.up[d]);
			leaves |= digs[d] != 1;
		}
		// a particle inside [lo, up) in every dimension is inside the frame
		// when 0 <= lo and up <= hi (thrInFrame): the frame test and the
		// in-place wrap only for the few that cross a threshold
		if (leaves || !thrInFrame) {
#pragma unroll
			for (int d = 0; d < ND; d++) {
				const double q = p[k][d] - (double)(digs[d] - 1) * (a.thr.hi[d] - 1.0);
				outside |= (q < 0.0 || q > a.thr.hi[d]);
				if ((a.wrapMask >> d) & 1) {
					if (digs[d] != 1) p[k][d] = p[k][d] + (double)((1 - digs[d]) * a.thr.T[d]);
					digs[d] = 1;
				}
			}
		}
#pragma unroll
		for (int d = ND - 1; d >= 0; d--) ne = ne * 3 + digs[d];
		// pPosAssertInLocalFrame fails for this particle (the host stops the
		// run with msg(ERROR) before the next deposit): route it to the
		// emigrant path so that nothing indexes the grid with it
		bad |= (int)outside << 1;
		if (outside) ne = 0;
		if (OBJ && ne == a.center) {
			// oCollectObjectCharge (object.c:489-494): the cell's lower node,
			// looked up only inside the objects' bounding box (which lies in
			// the node table: 32-bit index)
			bool inBB = true;
#pragma unroll
			for (int d = 0; d < ND; d++) inBB &= (unsigned)((int)p[k][d] - a.objLo[d]) <= (unsigned)a.objExt[d];
			unsigned node = (unsigned)(int)p[k][0];
			if (ND > 1) node += (unsigned)(int)p[k][1] * (unsigned)a.objSy;
			if (ND > 2) node += (unsigned)(int)p[k][2] * (unsigned)a.objSz;
			const int id = inBB ? a.objIn[node] : 0;
			if (id) {
				ne = PINC_NE_SINK;
				atomicAdd(&a.objCount[id - 1], 1);  // rare: particles entering an object
			}
		}
		if (SORT) {
			stageF[k * kPushThreads + threadIdx.x] = (unsigned char)ne;  // by item
		}
		// (sparse: the species' flags are the centre already -- the last
		// extraction put them back -- so only the leavers' are written, 1 B
		// per particle less at one rank, where every dimension wraps in place)
		if (!SORT && (!a.flagsSparse || ne != a.center)) a.flags[i] = (unsigned char)ne;
		if (ne != a.center) {
			cnt++;
		} else {
			dep |= (1u | (unsigned)chg << 16) << k;  // bits 16+: changed cell
		}
	}
	// (all pairs after the last kick: storing each pair right after its
	// kick, to free its velocity registers, measured 20.6 -> 26.2 ms per
	// plain push at C4, profiles/r05j_push_early_store_ab.txt)
	if (!SORT && full) {
		// the load's row swap backwards (an involution)
		const long q0 = base + wv * 256 + 2 * pi_lane((int)(threadIdx.x & 63));
		auto put = [&](double *o, const double (*q)[ND], int d) {
			dvec2 a0{q[0][d], q[1][d]}, a1{q[2][d], q[3][d]};
			rowswap(a0, a1);
			__builtin_nontemporal_store(a0, reinterpret_cast<dvec2 *>(o + q0));
			__builtin_nontemporal_store(a1, reinterpret_cast<dvec2 *>(o + q0 + 128));
		};
#pragma unroll
		for (int d = 0; d < ND; d++) {
			put(a.xo[d], p, d);
			if (wvel) put(a.vo[d], vv, d);
		}
	} else
	if (!SORT) {
#pragma unroll
		for (int k = 0; k < kPushItems; k += 2) store_pair(k);
	}
	PUSH_TS(4);
	if (SORT) {
		// global start of each brick's run (the reservation made before the kick)
		if ((int)threadIdx.x < ib.vol) bBase[threadIdx.x] = resBase;
		__syncthreads();
		// every item straight to its slot: the lanes of a wave instruction
		// that share a brick took consecutive ranks from its LDS counter, so
		// their stores cover one contiguous range (coalesced like the plain
		// push's) and no staging through LDS is needed
#pragma unroll
		for (int k = 0; k < kPushItems; k++) {
			if (!((valid >> k) & 1u)) continue;
			const long i = item(k);
			const int r = rlL[k * kPushThreads + threadIdx.x];
			const long o = r < 0      ? (long)~r
			               : cellRank ? (long)bBase[(r >> 4) & 63] + ccL[r & 1023] + (r >> 10)
			                          : (long)bBase[r & 255] + (r >> 8);
#pragma unroll
			for (int d = 0; d < ND; d++) {
				// (nontemporal, 8 B per lane: 24.4 -> 33.5 ms per sorting push,
				// profiles/r06i_count_runs_sort_nt_ab.txt)
				a.xo[d][o] = p[k][d];
				a.vo[d][o] = vv[k][d];
			}
			const int f = stageF[k * kPushThreads + threadIdx.x];
			if (!a.flagsSparse || f != a.center) a.flags[o] = (unsigned char)f;
			if (f != a.center) atomicAdd(&a.chunkCount[o / PINC_CHUNK], 1);
		}
	}
	PUSH_TS(5);
	if (a.cntNext) {
		// count the output bricks of the particles that stay (next push's
		// sort): a thread's consecutive items mostly share one, so the items in
		// the brick of its first counted item add once (plain LDS atomics)
		int l0 = -1, nm = 0;
#pragma unroll
		for (int k = 0; k < kPushItems; k++) {
			const bool mine = (dep >> k) & 1u;
			int c[3] = {0, 0, 0};
#pragma unroll
			for (int d = 0; d < ND; d++) c[d] = sort_cell(p[k][d], vv[k][d]);
			const int lb = mine ? brick_inside<ND>(a.tg, obb, c) : -1;
			if (lb >= 0 && l0 < 0) l0 = lb;
			if (lb >= 0 && lb == l0) nm++;
			else if (lb >= 0) atomicAdd(&cntOut[lb], 1);
			if (mine && lb < 0) atomicAdd(&a.cntNext[brick_first_key<ND>(a.tg, c)], 1);
		}
		if (nm) atomicAdd(&cntOut[l0], nm);
	}
	if (bad) atomicOr(a.err, bad);
	if (!SORT || a.emigTotal) {
		int wc = wave_sum_i(cnt);
		if (lane == 0) wcnt[wv] = wc;
	}
	if (a.moved) {
		int wm = wave_sum_i(__popc(dep >> 16));
		if (lane == 0) wmov[wv] = wm;
	}

	PUSH_TS(6);
	// ---- phase E: deposit of the particles that stay
	// global fallback of one corner (nodes outside the LDS box: far movers,
	// wrapped particles, a block whose box did not fit)
	auto add_corner_global = [&](const int *j, int c, double w) {
		int off = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			int o0, o1;
			node_pair(G, d, j[d], o0, o1);
			off += ((c >> d) & 1) ? o1 : o0;
		}
		unsafeAtomicAdd(&a.rho[(unsigned)off], w);
	};
	// LDS offsets of the 2^ND corners relative to the cell's lower node
	// (block-uniform: scalar registers)
	int coff[NC];
#pragma unroll
	for (int c = 0; c < NC; c++) {
		int o = 0, st = 1;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			o += ((c >> d) & 1) ? st : 0;
			st *= rB.n[d];
		}
		coff[c] = o;
	}
	// LDS index of the cell's lower node if all 2^ND corners lie in the box,
	// else -1 (one test per particle instead of one per corner)
	auto box_cell = [&](const int *j) -> int {
		bool in = rB.vol > 0;
#pragma unroll
		for (int d = 0; d < ND; d++) in &= (unsigned)(j[d] - rB.lo[d]) < (unsigned)(rB.n[d] - 1);
		return in ? rB.index(j, ND) : -1;
	};
	auto add8 = [&](const int *j, int l0, const double *w) {
		if (l0 >= 0) {
			l0 += myCopy;
#pragma unroll
			for (int c = 0; c < NC; c++) atomicAdd(&rhoL[l0 + coff[c]], w[c]);
		} else {
			if (a.diag) atomicAdd(&a.diag[2], 1ull);  // (trace: [2] += runs added to memory)
#pragma unroll
			for (int c = 0; c < NC; c++) add_corner_global(j, c, w[c]);
		}
	};
	const int keyMul[3] = {1, G.T[0] + 2, (G.T[0] + 2) * (G.T[1] + 2)};  // unique cell key
	// CIC weights and cell key of item k (a particle that stays)
	auto weights = [&](int k, int *j, double *w) -> int {
		double dec[3], comp[3];
		int kk = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			j[d] = (int)p[k][d];
			dec[d] = p[k][d] - j[d];
			comp[d] = 1 - dec[d];
			kk += d ? mul24(j[d], keyMul[d]) : j[d];
		}
		cic_weights<ND, V3D>(dec, comp, w);
		literal_ghost_weights<ND>(a.g, j, w);
		// the cell's periodic image nearest the block's reference cell (the
		// boxes' coordinates): a particle that wrapped deposits into the LDS
		// box at its image nodes, which the flush maps to the same storage
		// (x, y wrapped; slab ghost planes when the slab dimension wraps,
		// folded by the halo add as every ghost deposit) instead of adding
		// its eight weights to memory
		if (useImg) {
#pragma unroll
			for (int d = 0; d < ND; d++) j[d] = img(d, j[d]);
		}
		return kk;
	};
	// consecutive particles of the thread: runs of one cell are summed in
	// registers and added once (8 LDS atomics per run)
	{
		int jr[3] = {0, 0, 0}, keyr = -1;
		double wr[8];
		bool open = false;
#pragma unroll
		for (int k = 0; k < kPushItems; k++) {
			if (!((dep >> k) & 1u)) continue;
			int jk[3] = {0, 0, 0};
			double wk[8];
			const int kk = weights(k, jk, wk);
			if (open && kk == keyr) {
#pragma unroll
				for (int c = 0; c < 8; c++) wr[c] += wk[c];
			} else {
				if (open) add8(jr, box_cell(jr), wr);
				open = true;
				keyr = kk;
#pragma unroll
				for (int d = 0; d < 3; d++) jr[d] = jk[d];
#pragma unroll
				for (int c = 0; c < 8; c++) wr[c] = wk[c];
			}
		}
		if (open) add8(jr, box_cell(jr), wr);
	}

	if (KICK) {
		// per-wave sums with DPP (no LDS shuffles); the block barrier below
		// publishes them
		const double w = wave_sum_d(ke);
		if (lane == 0) kered[wv] = w;
	}
	__syncthreads();
	if (KICK && threadIdx.x == 0) {
		double t = 0.0;
		for (int w = 0; w < NW; w++) t += kered[w];
		a.kePartial[chunk] = t;
	}
	if ((!SORT || a.emigTotal) && threadIdx.x == 0) {
		int t = 0;
		for (int w = 0; w < NW; w++) t += wcnt[w];
		if (!SORT && t) atomicAdd(&a.chunkCount[base / PINC_CHUNK], t);  // zeroed by the caller
		if (t && a.emigTotal) atomicAdd(a.emigTotal, (unsigned long long)t);
	}
	if (a.moved && threadIdx.x == 0) {
		int t = 0;
		for (int w = 0; w < NW; w++) t += wmov[w];
		if (t) atomicAdd(a.moved, (unsigned long long)t);
	}
	if (a.spread && threadIdx.x == 0 && !empty) {
		unsigned long long v = 1;
#pragma unroll
		for (int d = 0; d < ND; d++) v *= (unsigned long long)(chi[d] - clo[d] + 1);
		atomicAdd(a.spread, v);
	}
	// flush: one global atomic per touched node / output cell
	const BoxRcp rq = box_rcp(rB);
	for (int t = threadIdx.x; t < rB.vol; t += kPushThreads) {
		double v = rhoL[t];
		for (int c = 1; c < nCopy; c++) v += rhoL[c * rStride + t];
		if (v == 0.0) continue;
		int c[3] = {0, 0, 0};
		box_coords(rB, rq, t, c, ND);
		int off = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			int o0, o1;
			node_pair(G, d, c[d], o0, o1);
			off += o0;
		}
		unsafeAtomicAdd(&a.rho[(unsigned)off], v);
	}
	if (a.cntNext) {
		for (int t = threadIdx.x; t < obb.vol; t += kPushThreads) {
			int m = cntOut[t];
			if (m) atomicAdd(&a.cntNext[brick_key<ND>(a.tg, obb, t)], m);
		}
	}
	// (trace: the last phase includes every wave's drain of its stores and
	// atomics)
	if (a.tstamp) {
		__builtin_amdgcn_s_waitcnt(0);
		__syncthreads();
	}
	PUSH_TS(7);
}

// rho = chain of the species accumulators with the reference's rescaling
// (gZero; per species gMul(1/q), add, gMul(q); pusher.c:512-572)
struct CombineArgs {
	const double *acc[PINC_MAX_SPECIES];
	double q[PINC_MAX_SPECIES];
	int ns;
};

__global__ void k_rho_combine(double *__restrict__ rho, CombineArgs c, long n) {
	for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
		double r = c.acc[0][i];
		for (int s = 1; s < c.ns; s++) r = (r * c.q[s - 1]) * (1.0 / c.q[s]) + c.acc[s][i];
		rho[i] = r * c.q[c.ns - 1];
	}
}

// ------------------------------------------------- order 0 (NGP) ---------
// puDistrND0 (pusher.c:640-668) and puAccND0KE (pusher.c:310-353) with
// puInterpND0 (pusher.c:1164-1180): the nearest node (int)(x + 0.5) of the
// padded local frame takes the whole particle (one unit; the caller applies
// the species' 1/q, q chain) and lends it its E.  Not on the hot path (main.c
// offers them through select; the configs use CIC): one thread per particle,
// global atomics.
template <int ND>
__global__ __launch_bounds__(kThreads) void k_deposit_ngp(const double *__restrict__ x0,
                                                          const double *__restrict__ x1,
                                                          const double *__restrict__ x2, long b0, long n,
                                                          pinc_geom_t g, double *__restrict__ rho) {
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
		int j[3] = {0, 0, 0};
		long off = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			j[d] = (int)(xs[d][b0 + i] + 0.5);
			off += node_off(G, d, j[d]);
		}
		const double w = g.literal ? literal_node_factor<ND>(g, j) : 1.0;
		if (w != 0.0) unsafeAtomicAdd(&rho[off], w);
	}
}

template <int ND>
__global__ __launch_bounds__(kThreads) void k_accel_ngp(const double *__restrict__ x0, const double *__restrict__ x1,
                                                        const double *__restrict__ x2, double *__restrict__ v0,
                                                        double *__restrict__ v1, double *__restrict__ v2, long b0,
                                                        long n, pinc_geom_t g, const double *__restrict__ E,
                                                        double *__restrict__ kePartial) {
	__shared__ double red[kThreads / 64];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	double *vs[3] = {v0, v1, v2};
	double ke = 0.0;
	// block b owns particles [b kAccChunk, (b+1) kAccChunk): the KE partials
	// have pinc_hip_accelerate's layout
	for (int k = 0; k < kAccItems; k++) {
		const long i = (long)blockIdx.x * kAccChunk + (long)k * kThreads + threadIdx.x;
		if (i >= n) break;
		long off = 0;
#pragma unroll
		for (int d = 0; d < ND; d++) off += node_off(G, d, (int)(xs[d][b0 + i] + 0.5));
		off *= ND;
		double vsq = 0.0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			const double dv = E[off + d];
			const double vv = vs[d][b0 + i];
			vsq += vv * (vv + dv);
			vs[d][b0 + i] = vv + dv;
		}
		ke += vsq;
	}
	const double t = block_sum(ke, red);
	if (threadIdx.x == 0) kePartial[blockIdx.x] = t;
}

// ------------------------------------- order 2 (quadratic spline) ---------
// puDistrND2 / puAccND2KE (an extension; the reference's puSanity anticipates
// order 2, pusher.c:1047-1087): the quadratic B-spline over the nearest true
// node j and its two neighbours per dimension, the rule of include/pinc_hip.h.
// j is clamped to 1..T, so the stencil stays on the padded nodes 0..T+1
// whatever the position holds.

// nearest true node j[d] and the three one-dimensional weights w1[d][0..2] of
// nodes j-1, j, j+1; true if j is the node cj of the thread's current run
template <int ND>
__device__ __forceinline__ bool tsc_split(const double *x, const int *T, const int *cj, int *j, double (*w1)[3]) {
	bool same = true;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		j[d] = min(max((int)(x[d] + 0.5), 1), T[d]);
		const double dl = x[d] - j[d];
		const double a = 0.5 - dl, b = 0.5 + dl;
		w1[d][0] = 0.5 * (a * a);
		w1[d][1] = 0.75 - dl * dl;
		w1[d][2] = 0.5 * (b * b);
		same = same && (j[d] == cj[d]);
	}
	return same;
}

// stencil index of node c = i0 + 3 i1 + 9 i2 along dimension d (0..2: j-1..j+1)
__device__ __forceinline__ constexpr int tsc_digit(int c, int d) { return d == 0 ? c % 3 : d == 1 ? (c / 3) % 3 : c / 9; }

// the 3^ND node weights, the product taken in the order d = ND-1 .. 0 as
// cic_weights' general form
template <int ND>
__device__ __forceinline__ void tsc_weights(const double (*w1)[3], double *w) {
	constexpr int NN = ND == 3 ? 27 : ND == 2 ? 9 : 3;
#pragma unroll
	for (int c = 0; c < NN; c++) {
		double f = 1.0;
#pragma unroll
		for (int d = ND - 1; d >= 1; d--) f = w1[d][tsc_digit(c, d)] * f;
		w[c] = w1[0][tsc_digit(c, 0)] * f;
	}
}

// the same for the nodes of one layer: index c = i0 + 3 i1 within the layer lz
// of the last dimension in 3-D (c alone below that)
__device__ __forceinline__ int tsc_layer_digit(int c, int lz, int d) { return d == 2 ? lz : tsc_digit(c, d); }
template <int ND>
__device__ __forceinline__ void tsc_layer_weights(const double (*w1)[3], int lz, double *w) {
	if constexpr (ND < 3) {
		tsc_weights<ND>(w1, w);
	} else {
		const double wz = lz == 0 ? w1[2][0] : lz == 1 ? w1[2][1] : w1[2][2];
#pragma unroll
		for (int c = 0; c < 9; c++) w[c] = w1[0][c % 3] * (w1[1][c / 3] * wz);
	}
}

// global offset of stencil node c of the stencil centred on padded node j
template <int ND>
__device__ __forceinline__ long tsc_node_off(const Geo &G, const int *j, int c) {
	long off = 0;
#pragma unroll
	for (int d = 0; d < ND; d++) off += node_off(G, d, j[d] - 1 + tsc_digit(c, d));
	return off;
}

// k_deposit_tiled's frame with the three-node stencil: the chunk's box spans
// [min j - 1, max j + 1] per dimension; a run of consecutive particles with one
// nearest node is summed in 3^ND registers and added once.
template <int ND>
__global__ __launch_bounds__(kThreads) void k_deposit_tsc(const double *__restrict__ x0,
                                                          const double *__restrict__ x1,
                                                          const double *__restrict__ x2, long b0, long n,
                                                          pinc_geom_t g, double *__restrict__ rho) {
	constexpr int NN = ND == 3 ? 27 : ND == 2 ? 9 : 3;
	g.nd = ND;  // (the launcher's choice of instance, here a constant: the slab dimension folds)
	__shared__ double acc[kDepCap];
	__shared__ BlockBounds<3, false, false> bounds;
	__shared__ int box[7];
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	const ChunkItems<kDepItems> ch(b0, n);

	// pass 1: bounds of the chunk's nearest nodes
	int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
#pragma unroll
	for (int d = 0; d < ND; d++) {
#pragma unroll
		for (int k = 0; k < kDepItems; k += 2) {
			double x[2];
			ch.load2(xs[d], k, x[0], x[1]);
#pragma unroll
			for (int h = 0; h < 2; h++)
				if (ch.live(k + h)) {
					const int c = min(max((int)(x[h] + 0.5), 1), G.T[d]);
					lo[d] = min(lo[d], c);
					hi[d] = max(hi[d], c);
				}
		}
	}
	bounds.reduce(ND, lo, hi, nullptr, 0);
	if (threadIdx.x == 0) {
		long vol = 1;
		for (int d = 0; d < ND; d++) {
			int a, b, s;
			bounds.get(d, a, b, s);
			box[d] = a - 1;
			box[3 + d] = b - a + 3;
			vol *= (long)(b - a + 3);
		}
		box[6] = (vol <= kDepCap && vol > 0) ? (int)vol : 0;
	}
	__syncthreads();

	NodeBox<ND> nb;
	if (box[6]) {
		nb = NodeBox<ND>(box, box + 3);
		nb.zero(acc, 1);
		__syncthreads();
	}

	// pass 2: runs of equal nearest nodes summed in registers, NA nodes at a
	// time: all 3^ND in 1-D and 2-D, one z-layer of nine per pass over the
	// thread's particles in 3-D (27 accumulators next to 27 weights and the
	// adds' addresses took 248 VGPRs and spilled scalar registers; the
	// particles of the later passes come from cache).  One particle per turn
	// and one more turn for the last run, so that a run's adds are in the
	// code once; pairs are still loaded 16 B wide.
	constexpr int NL = ND == 3 ? 3 : 1, NA = NN / NL;
#pragma unroll 1
	for (int lz = 0; lz < NL; lz++) {
		int cj[3] = {INT32_MIN, 0, 0};
		double a[NA];
#pragma unroll
		for (int c = 0; c < NA; c++) a[c] = 0.0;
		double pp[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll 1
		for (int k = 0; k <= kDepItems; k++) {
			const bool last = k == kDepItems;
			if (!last && !(k & 1)) {
#pragma unroll
				for (int d = 0; d < ND; d++) ch.load2(xs[d], k, pp[0][d], pp[1][d]);
			}
			const bool lv = !last && ch.live(k);
			if (!last && !lv) continue;
			// (On the extra turn x is the last pair again and lv is false: j is
			// clamped, so nothing is out of range, `same` is false and the weights
			// are dropped.  Skipping their computation under `if (lv)` costs the
			// 3-D instance 49 VGPRs and a wave of occupancy, so it stays.)
			double x[3], w1[3][3], w[NA];
			int j[3];
#pragma unroll
			for (int d = 0; d < ND; d++) x[d] = (k & 1) ? pp[1][d] : pp[0][d];
			const bool same = tsc_split<ND>(x, G.T, cj, j, w1) && lv;
			tsc_layer_weights<ND>(w1, lz, w);
			if (g.literal) {
#pragma unroll
				for (int c = 0; c < NA; c++) {
					int p[3];
#pragma unroll
					for (int d = 0; d < ND; d++) p[d] = j[d] - 1 + tsc_layer_digit(c, lz, d);
					w[c] *= literal_node_factor<ND>(g, p);
				}
			}
			if (same) {
#pragma unroll
				for (int c = 0; c < NA; c++) a[c] += w[c];
				continue;
			}
			// the run ends: add it (the bounding box holds every run's stencil)
			if (cj[0] != INT32_MIN) {
				if (nb.vol) {
					int l;
					nb.index_centre(cj, l);
#pragma unroll
					for (int c = 0; c < NA; c++) {
						int off = l;
#pragma unroll
						for (int d = 0; d < ND; d++) off += (tsc_layer_digit(c, lz, d) - 1) * nb.st[d];
						atomicAdd(&acc[off], a[c]);
					}
				} else {
#pragma unroll
					for (int c = 0; c < NA; c++) {
						long off = 0;
#pragma unroll
						for (int d = 0; d < ND; d++) off += node_off(G, d, cj[d] - 1 + tsc_layer_digit(c, lz, d));
						unsafeAtomicAdd(&rho[off], a[c]);
					}
				}
			}
#pragma unroll
			for (int c = 0; c < NA; c++) a[c] = w[c];
#pragma unroll
			for (int d = 0; d < ND; d++) cj[d] = j[d];
		}
	}
	if (!nb.vol) return;
	__syncthreads();
	nb.flush(acc, 1, G, rho);
}

// k_accel_ngp's chunking and KE partials; dv_d = sum over the 3^ND nodes of
// w Es[node ND + d], nodes in the order c = 0 .. 3^ND - 1, gathered through L2
template <int ND>
__global__ __launch_bounds__(kThreads) void k_accel_tsc(const double *__restrict__ x0, const double *__restrict__ x1,
                                                        const double *__restrict__ x2, double *__restrict__ v0,
                                                        double *__restrict__ v1, double *__restrict__ v2, long b0,
                                                        long n, pinc_geom_t g, const double *__restrict__ E,
                                                        double *__restrict__ kePartial) {
	constexpr int NN = ND == 3 ? 27 : ND == 2 ? 9 : 3;
	__shared__ double red[kThreads / 64];
	g.nd = ND;
	Geo G = make_geo(g);
	const double *xs[3] = {x0, x1, x2};
	double *vs[3] = {v0, v1, v2};
	const int none[3] = {0, 0, 0};
	double ke = 0.0;
	for (int k = 0; k < kAccItems; k++) {
		const long i = (long)blockIdx.x * kAccChunk + (long)k * kThreads + threadIdx.x;
		if (i >= n) break;
		double x[3], w1[3][3], w[NN], dv[3] = {0.0, 0.0, 0.0};
		int j[3];
#pragma unroll
		for (int d = 0; d < ND; d++) x[d] = xs[d][b0 + i];
		tsc_split<ND>(x, G.T, none, j, w1);
		tsc_weights<ND>(w1, w);
#pragma unroll
		for (int c = 0; c < NN; c++) {
			const long off = tsc_node_off<ND>(G, j, c) * ND;
#pragma unroll
			for (int d = 0; d < ND; d++) dv[d] += w[c] * E[off + d];
		}
		double vsq = 0.0;
#pragma unroll
		for (int d = 0; d < ND; d++) {
			const double vv = vs[d][b0 + i];
			vsq += vv * (vv + dv[d]);
			vs[d][b0 + i] = vv + dv[d];
		}
		ke += vsq;
	}
	const double t = block_sum(ke, red);
	if (threadIdx.x == 0) kePartial[blockIdx.x] = t;
}

// pVelAssertMax (population.c:342-365): a component above maxVel (signed, as
// the reference) sets bit 0 of the assert word
__global__ __launch_bounds__(kThreads) void k_vel_assert(const double *__restrict__ v0, const double *__restrict__ v1,
                                                         const double *__restrict__ v2, long b0, long n, int nd,
                                                         double maxVel, int *__restrict__ err) {
	const double *vs[3] = {v0, v1, v2};
	int bad = 0;
	for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
		for (int d = 0; d < nd; d++) bad |= vs[d][b0 + i] > maxVel;
	if (bad) atomicOr(err, 1);
}

// ------------------------------------------------------- collisions -------
// Monte Carlo collisions with a neutral background (an extension; the rule is
// in include/pinc_hip.h).  A workgroup owns kColChunk consecutive slots from
// the 16-byte aligned slot at or below iStart.  Only velocities are touched.
// Draws are counters of the species-local index, so a particle's outcome does
// not depend on which thread holds it.  Two instances per dimension count,
// chosen by the launch's parameters:
//  * EAGER (some sig != 0): the collision probability depends on the
//    particle's speed relative to its neutral, so every particle's neutral is
//    sampled.  The chunk frame of k_accel: velocities read as lane-contiguous
//    16-B pairs;
//  * otherwise the probability is the same for every particle and one draw
//    decides, without the velocity.  Pass 1 makes that draw for every slot and
//    lists the colliders' slots in LDS; pass 2 deals the list out densely, one
//    collider per lane, and only there are velocities read and the neutral
//    sampled.  (Deciding and colliding in one per-lane pass makes a wave run
//    the whole collision branch whenever one of its 64 lanes collides: at 1 %
//    colliding that is 1 - 0.99^64 = 0.47 of all wave iterations, and the
//    launch took 1.62 ms of which 1.05 above a plain read, 0.47 of the eager
//    form's 2.25.)
// A collider's components are stored one by one (8 B per lane): nothing is
// written for a particle that did not collide.  Measured against storing the
// whole 16-B pair when either half collided, in a variant build of the
// one-pass form (DESIGN.md section 4 "Collisions"; 128^3, 64 ppc): 1.62
// against 1.63-1.64 ms with 1 % colliding, 2.82-2.85 either way in
// cross-section mode, 3.28-3.34 against 3.19 ms with 63 % colliding: the pair
// form wins only where most particles collide, which is not the regime the
// operator is for.  The two counts are summed per wave (DPP), per block (LDS),
// and added with one atomic per block and process that is not zero.
constexpr int kColItems = 8;
constexpr int kColChunk = kThreads * kColItems;

// one particle: v[0..ND) in, and out if it collides; returns the process
// (0 elastic, 1 charge exchange) or -1
template <int ND>
__device__ __forceinline__ int collide_one(const pinc_collide_t &c, unsigned long long base, double *v) {
	const double u0 = uni(c.key, base);
	double nn[ND], w[ND];
	{
		double sn, cs;
		const double R = sqrt(-2.0 * log(uni(c.key, base + 4)));
		sincospi(2.0 * uni(c.key, base + 5), &sn, &cs);
		nn[0] = c.drift[0] + c.vth * (R * cs);
		if constexpr (ND > 1) nn[1] = c.drift[1] + c.vth * (R * sn);
		if constexpr (ND > 2)
			nn[2] = c.drift[2] + c.vth * (sqrt(-2.0 * log(uni(c.key, base + 6))) * cospi(2.0 * uni(c.key, base + 7)));
	}
	double g2 = 0.0;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		w[d] = c.h[d] * v[d];
		const double gd = w[d] - nn[d];
		g2 += gd * gd;
	}
	const double g = sqrt(g2);
	const double r0 = c.nu[0] + c.sig[0] * g, r1 = c.nu[1] + c.sig[1] * g, r = r0 + r1;
	if (!(u0 < -expm1(-r))) return -1;
	if (!(uni(c.key, base + 1) * r < r0)) {
#pragma unroll
		for (int d = 0; d < ND; d++) v[d] = nn[d] / c.h[d];
		return 1;
	}
	double e[ND];
	const double u2 = uni(c.key, base + 2);
	if constexpr (ND == 3) {
		double sn, cs;
		const double ct = 1.0 - 2.0 * u2, st = sqrt((1.0 - ct) * (1.0 + ct));
		sincospi(2.0 * uni(c.key, base + 3), &sn, &cs);
		e[0] = st * cs;
		e[1] = st * sn;
		e[2] = ct;
	} else if constexpr (ND == 2) {
		sincospi(2.0 * u2, &e[1], &e[0]);
	} else {
		e[0] = u2 < 0.5 ? 1.0 : -1.0;
	}
	const double a = 1.0 - c.b, bg = c.b * g;
#pragma unroll
	for (int d = 0; d < ND; d++) v[d] = ((a * w[d] + c.b * nn[d]) + bg * e[d]) / c.h[d];
	return 0;
}

template <int ND, bool EAGER>
__global__ __launch_bounds__(kThreads) void k_collide(double *__restrict__ v0, double *__restrict__ v1,
                                                      double *__restrict__ v2, long b0, long n, pinc_collide_t c,
                                                      unsigned long long *__restrict__ counts) {
	__shared__ int red[2 * kWaves];
	// the parameters are read from LDS, into vector registers where they are
	// used: held in scalar registers for the whole kernel, next to the
	// constants of log, expm1 and sincospi, they spill scalar registers in 3-D
	__shared__ pinc_collide_t par;
	__shared__ int list[EAGER ? 1 : kColChunk];  // slots of the chunk's colliders
	__shared__ int nList;
	if (threadIdx.x == 0) {
		par = c;
		nList = 0;
	}
	__syncthreads();
	double *vs[3] = {v0, v1, v2};
	const long end = b0 + n;
	const long chunk0 = (b0 & ~1L) + (long)blockIdx.x * kColChunk;
	int nEl = 0, nCx = 0;
	if constexpr (EAGER) {
		const long cb = chunk0 + 2L * threadIdx.x;
#pragma unroll
		for (int k = 0; k < kColItems; k += 2) {
			const long i = cb + 2L * kThreads * (k >> 1);
			const bool ok[2] = {i >= b0 && i < end, i + 1 >= b0 && i + 1 < end};
			if (!ok[0] && !ok[1]) continue;
			double v[2][ND];
#pragma unroll
			for (int d = 0; d < ND; d++) {
				if (ok[0] && ok[1]) {
					const double2 t = *reinterpret_cast<const double2 *>(vs[d] + i);
					v[0][d] = t.x;
					v[1][d] = t.y;
				} else {
					v[0][d] = v[1][d] = vs[d][ok[0] ? i : i + 1];
				}
			}
#pragma unroll
			for (int h = 0; h < 2; h++) {
				if (!ok[h]) continue;
				const int proc = collide_one<ND>(par, 8ull * (unsigned long long)(i + h - b0), v[h]);
				if (proc < 0) continue;
				nEl += proc == 0;
				nCx += proc == 1;
#pragma unroll
				for (int d = 0; d < ND; d++) vs[d][i + h] = v[h][d];
			}
		}
	} else {
		// pass 1: r = nu_0 + nu_1 for every particle (sig_k g adds an exact
		// zero), so P is the launch's, formed once with the rule's expression
		const double P = -expm1(-(c.nu[0] + c.nu[1]));
#pragma unroll
		for (int k = 0; k < kColItems; k++) {
			const int slot = k * kThreads + threadIdx.x;
			const long i = chunk0 + slot;
			if (i >= b0 && i < end && uni(c.key, 8ull * (unsigned long long)(i - b0)) < P) list[atomicAdd(&nList, 1)] = slot;
		}
		__syncthreads();
		// pass 2: the colliders, one per lane (collide_one repeats the
		// decision with the particle's own r: the same bits for a finite
		// velocity, and no collision for one that is not)
		// (unrolled: as a loop, the fp64 constants of log, expm1 and sincospi
		// are hoisted out of it and held in 128 VGPRs and spilled SGPRs)
		const int nl = nList;
#pragma unroll
		for (int q = 0; q < kColItems; q++) {
			const int t = q * kThreads + threadIdx.x;
			if (t >= nl) break;
			const long i = chunk0 + list[t];
			double v[ND];
#pragma unroll
			for (int d = 0; d < ND; d++) v[d] = vs[d][i];
			const int proc = collide_one<ND>(par, 8ull * (unsigned long long)(i - b0), v);
			if (proc < 0) continue;
			nEl += proc == 0;
			nCx += proc == 1;
#pragma unroll
			for (int d = 0; d < ND; d++) vs[d][i] = v[d];
		}
	}
	// (every lane of every wave arrives here: the DPP sums need them all)
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
	for (int p = 0; p < 2; p++) {
		const int t = wave_sum_i(p ? nCx : nEl);
		if (lane == 0) red[p * kWaves + wv] = t;
	}
	__syncthreads();
	if (threadIdx.x < 2) {
		int t = 0;
		for (int q = 0; q < kWaves; q++) t += red[threadIdx.x * kWaves + q];
		if (t) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
	}
}

// ------------------------------------------------------- ionisation -------
// Electron-impact ionisation against the same neutral background (an
// extension; the rule is in include/pinc_hip.h).  The one process that creates
// particles: birth k of a launch, counted in ascending parent index, puts an
// electron at slot iStop[s] + k and an ion at iStop[target] + k.  That order
// needs every block's first k before anything is written, so the kernel runs
// twice around a scan of the blocks' counts (pinc_hip_ionize):
//  * WRITE = false decides every particle and writes the block's births;
//  * WRITE = true tests the total against the free slots of both species (a
//    launch that does not fit writes nothing but res[1]), decides again -- the
//    draws are counters, the arithmetic is the same code: the same bits --
//    and ranks the births of an item by a wave ballot and the waves' counts
//    in LDS, the items in turn.
// A workgroup owns kIonChunk consecutive slots in k_collide's frame; item q of
// thread t is slot q kThreads + t, so that items, waves and lanes ascend with
// the index.  Two instances of each, chosen as k_collide's:
//  * EAGER (sig != 0): the probability depends on the particle's speed, so
//    every live slot is an entry of the second stage;
//  * otherwise u0 < P, with the launch's one P, is necessary: the first stage
//    makes that draw alone and lists the candidates in LDS in index order
//    (the same ballot ranking), and the second stage deals them out densely,
//    so that the neutral's logarithms and the threshold test run on full
//    waves (the reason is k_collide's, measured there).
// The second stage is unrolled and the parameters come from LDS for the
// register reasons given at k_collide.
constexpr int kIonItems = 8;
constexpr int kIonChunk = kThreads * kIonItems;

// the ranges of one launch: live particles [b0, b0 + n) of the projectile, the
// first free slot of the projectile and of the target and their free slots
struct IonSpan {
	long b0, n, dstS, dstT, freeS, freeT;
};

// step 5's unit vector from the draws at counters cb and cb + 1
template <int ND>
__device__ __forceinline__ void ion_unit(unsigned long long key, unsigned long long cb, double *e) {
	const double ua = uni(key, cb);
	if constexpr (ND == 3) {
		double sn, cs;
		const double ct = 1.0 - 2.0 * ua, st = sqrt((1.0 - ct) * (1.0 + ct));
		sincospi(2.0 * uni(key, cb + 1), &sn, &cs);
		e[0] = st * cs;
		e[1] = st * sn;
		e[2] = ct;
	} else if constexpr (ND == 2) {
		sincospi(2.0 * ua, &e[1], &e[0]);
	} else {
		e[0] = ua < 0.5 ? 1.0 : -1.0;
	}
}

// steps 1 to 3 for one particle of velocity v: its neutral nn and, if it
// ionises, rem = G - W
template <int ND>
__device__ __forceinline__ bool ion_decide(const pinc_ionize_t &c, unsigned long long base, const double *v, double *nn,
                                           double &rem) {
	const double u0 = uni(c.key, base);
	{
		double sn, cs;
		const double R = sqrt(-2.0 * log(uni(c.key, base + 4)));
		sincospi(2.0 * uni(c.key, base + 5), &sn, &cs);
		nn[0] = c.drift[0] + c.vth * (R * cs);
		if constexpr (ND > 1) nn[1] = c.drift[1] + c.vth * (R * sn);
		if constexpr (ND > 2)
			nn[2] = c.drift[2] + c.vth * (sqrt(-2.0 * log(uni(c.key, base + 6))) * cospi(2.0 * uni(c.key, base + 7)));
	}
	double G = 0.0;
#pragma unroll
	for (int d = 0; d < ND; d++) {
		const double gd = c.h[d] * v[d] - nn[d];
		G += gd * gd;
	}
	const double r = c.nu + c.sig * sqrt(G), W = c.wth * c.wth;
	if (!(G > W && u0 < -expm1(-r))) return false;
	rem = G - W;
	return true;
}

template <int ND, bool EAGER, bool WRITE>
__global__ __launch_bounds__(kThreads) void k_ionize(double *__restrict__ x0, double *__restrict__ x1,
                                                     double *__restrict__ x2, double *__restrict__ v0,
                                                     double *__restrict__ v1, double *__restrict__ v2, IonSpan sp,
                                                     pinc_ionize_t c, int *__restrict__ counts,
                                                     const int *__restrict__ offsets, int nb,
                                                     unsigned long long *__restrict__ res) {
	__shared__ pinc_ionize_t par;
	__shared__ int list[EAGER ? 1 : kIonChunk];  // slots of the chunk's candidates, ascending
	__shared__ int cnt[kIonItems * kWaves];      // candidates per item and wave
	__shared__ int wcnt[2][kWaves];              // births per wave of an item (even and odd items)
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	int run = 0;  // births before the current item: of the launch (WRITE), of this thread (otherwise)
	if constexpr (WRITE) {
		// (the same for every block: all of them leave, or none)
		const long total = offsets[nb];
		if (total > sp.freeS || total > sp.freeT) {
			if (blockIdx.x == 0 && threadIdx.x == 0) res[1] = 1;
			return;
		}
		if (blockIdx.x == 0 && threadIdx.x == 0 && total) atomicAdd(&res[0], (unsigned long long)total);
		run = offsets[blockIdx.x];
	}
	if (threadIdx.x == 0) par = c;
	__syncthreads();
	double *xs[3] = {x0, x1, x2}, *vs[3] = {v0, v1, v2};
	const long end = sp.b0 + sp.n;
	const long chunk0 = (sp.b0 & ~1L) + (long)blockIdx.x * kIonChunk;
	int nl = kIonChunk;  // entries of the second stage
	if constexpr (!EAGER) {
		// r = nu for every particle (sig g adds an exact zero), so P is the
		// launch's, formed once with the rule's expression
		const double P = -expm1(-c.nu);
		unsigned mask = 0;
#pragma unroll
		for (int k = 0; k < kIonItems; k++) {
			const long i = chunk0 + k * kThreads + threadIdx.x;
			const bool cand = i >= sp.b0 && i < end && uni(c.key, 16ull * (unsigned long long)(i - sp.b0)) < P;
			const unsigned long long bal = __ballot(cand);
			if (lane == 0) cnt[k * kWaves + wv] = __popcll(bal);
			mask |= (unsigned)cand << k;
		}
		__syncthreads();
		nl = 0;
#pragma unroll
		for (int k = 0; k < kIonItems; k++) {
			const bool cand = (mask >> k) & 1;
			const unsigned long long bal = __ballot(cand);
			int before = 0, tot = 0;
#pragma unroll
			for (int q = 0; q < kWaves; q++) {
				before += q < wv ? cnt[k * kWaves + q] : 0;
				tot += cnt[k * kWaves + q];
			}
			if (cand) list[nl + before + __popcll(bal & lanemask_lt())] = k * kThreads + threadIdx.x;
			nl += tot;
		}
		__syncthreads();
	}
	// second stage: one entry per lane (ion_decide repeats a candidate's
	// decision with the particle's own r: the same bits for a finite velocity,
	// and no birth for one that is not)
#pragma unroll
	for (int q = 0; q < kIonItems; q++) {
		if (q * kThreads >= nl) break;  // (the same for the whole block)
		const int t = q * kThreads + threadIdx.x;
		long i = -1;
		if constexpr (EAGER) {
			if (chunk0 + t >= sp.b0 && chunk0 + t < end) i = chunk0 + t;
		} else {
			if (t < nl) i = chunk0 + list[t];
		}
		bool hit = false;
		double nn[ND], rem = 0.0;
		if (i >= 0) {
			double v[ND];
#pragma unroll
			for (int d = 0; d < ND; d++) v[d] = vs[d][i];
			hit = ion_decide<ND>(par, 16ull * (unsigned long long)(i - sp.b0), v, nn, rem);
		}
		if constexpr (!WRITE) {
			run += hit;
		} else {
			const unsigned long long bal = __ballot(hit);
			if (lane == 0) wcnt[q & 1][wv] = __popcll(bal);
			__syncthreads();
			int before = 0, tot = 0;
#pragma unroll
			for (int w = 0; w < kWaves; w++) {
				before += w < wv ? wcnt[q & 1][w] : 0;
				tot += wcnt[q & 1][w];
			}
			if (hit) {
				const long k = (long)run + before + __popcll(bal & lanemask_lt());
				const unsigned long long base = 16ull * (unsigned long long)(i - sp.b0);
				const double f = uni(par.key, base + 1);
				const double g1 = sqrt(f * rem), g2 = sqrt((1.0 - f) * rem);
				double e1[ND], e2[ND];
				ion_unit<ND>(par.key, base + 2, e1);
				ion_unit<ND>(par.key, base + 8, e2);
#pragma unroll
				for (int d = 0; d < ND; d++) {
					const double x = xs[d][i];
					vs[d][i] = (nn[d] + g1 * e1[d]) / par.h[d];
					xs[d][sp.dstS + k] = x;
					vs[d][sp.dstS + k] = (nn[d] + g2 * e2[d]) / par.h[d];
					xs[d][sp.dstT + k] = x;
					vs[d][sp.dstT + k] = nn[d] / par.h[d];
				}
			}
			run += tot;
		}
	}
	if constexpr (!WRITE) {
		// (every lane of every wave arrives here: the DPP sum needs them all)
		const int t = wave_sum_i(run);
		if (lane == 0) wcnt[0][wv] = t;
		__syncthreads();
		if (threadIdx.x == 0) {
			int s = 0;
			for (int w = 0; w < kWaves; w++) s += wcnt[0][w];
			counts[blockIdx.x] = s;
		}
	}
}

}  // namespace

// =========================================================== C ABI ========
// Every entry point marshals its arguments and launches one instance chosen
// by with_nd; species_span and upto_nd (common.h) form the particle range and
// the per-dimension pointers.

// the classification thresholds from the host's thr[3 * nd] (lower, upper,
// upper limit of each dimension); T is the number of true cells
static Thr make_thr(const double *thr, int nd) {
	Thr t;
	for (int d = 0; d < 3; d++) {
		t.lo[d] = d < nd ? thr[d] : 0;
		t.up[d] = d < nd ? thr[nd + d] : 0;
		t.hi[d] = d < nd ? thr[2 * nd + d] : 0;
		t.T[d] = d < nd ? (int)(thr[2 * nd + d] - 1.0 + 0.5) : 1;
	}
	return t;
}

// the neighbour code of a particle that stays: digit 1 in every dimension
static int flag_center(int nd) {
	int center = 0;
	for (int d = 0, p = 1; d < nd; d++, p *= 3) center += p;
	return center;
}

// multi-block scan of counts[0, n) into offsets (a single workgroup takes
// ~0.7 ms for 5e5 values); work: block sums[nsb] | block offsets[nsb + 1],
// nsb = ceil(n / kScanBlock)
static void scan_ints(const int *counts, long n, int *offsets, int *work, hipStream_t st) {
	const long nsb = ceil_div(n, (long)kScanBlock);
	int *bsum = work, *boff = work + nsb;
	hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nsb), dim3(kThreads), 0, st, counts, n, bsum);
	hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, bsum, boff, (int)nsb);
	hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nsb), dim3(kThreads), 0, st, counts, n, boff, offsets);
}

extern "C" long pinc_hip_push_chunk(void) { return kPushChunk; }

extern "C" int pinc_hip_push_xcd_of_chunks(long nBlocks, int *xcd) {
	for (long b = 0; b < nBlocks; b++) xcd[push_chunk_of((unsigned)nBlocks, (unsigned)b)] = (int)(b & 7);
	return 0;
}

extern "C" int pinc_hip_deposit_ngp(pinc_pop_t pop, int s, pinc_geom_t g, double *rho, void *stream) {
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = ceil_div(sp.n, (long)kThreads);
	if (nb > 65536) nb = 65536;
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_deposit_ngp<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, sp.b0, sp.n, g, rho);
	});
	return check_launch("deposit (NGP)");
}

extern "C" int pinc_hip_accelerate_ngp(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, double *kePartial,
                                       int *nBlocks, void *stream) {
	const Span sp = species_span(pop, s);
	*nBlocks = 0;
	if (sp.n <= 0) return 0;
	long nb = ceil_div(sp.n, (long)kAccChunk);
	*nBlocks = (int)nb;
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd), v = upto_nd(pop.v, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_accel_ngp<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c, sp.b0, sp.n,
		                   g, Es, kePartial);
	});
	return check_launch("accelerate (NGP)");
}

// a species index and dimensions the order-2 entry points accept
static int tsc_args_ok(const pinc_pop_t &pop, int s, const pinc_geom_t &g) {
	if (g.nd < 1 || g.nd > 3 || s < 0 || s >= PINC_MAX_SPECIES || s >= pop.nSpecies) return 0;
	for (int d = 0; d < g.nd; d++)
		if (!pop.x[d] || g.T[d] < 1) return 0;
	return g.nloc >= 1;
}

extern "C" int pinc_hip_deposit_tsc(pinc_pop_t pop, int s, pinc_geom_t g, double *rho, void *stream) {
	if (!tsc_args_ok(pop, s, g) || !rho)
		return set_error(hipErrorInvalidValue, "deposit (order 2): bad species, dimensions or null array");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = chunk_blocks(sp.b0, sp.n, kDepChunk);
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_deposit_tsc<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, sp.b0, sp.n, g, rho);
	});
	return check_launch("deposit (order 2)");
}

extern "C" int pinc_hip_accelerate_tsc(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, double *kePartial,
                                       int *nBlocks, void *stream) {
	if (nBlocks) *nBlocks = 0;
	if (!tsc_args_ok(pop, s, g) || !Es || !kePartial || !nBlocks)
		return set_error(hipErrorInvalidValue, "accelerate (order 2): bad species, dimensions or null array");
	for (int d = 0; d < g.nd; d++)
		if (!pop.v[d]) return set_error(hipErrorInvalidValue, "accelerate (order 2): null velocity array");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = ceil_div(sp.n, (long)kAccChunk);
	*nBlocks = (int)nb;
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd), v = upto_nd(pop.v, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_accel_tsc<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c, sp.b0, sp.n,
		                   g, Es, kePartial);
	});
	return check_launch("accelerate (order 2)");
}

extern "C" int pinc_hip_vel_assert(pinc_pop_t pop, int s, double maxVel, int *errFlag, void *stream) {
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = ceil_div(sp.n, (long)kThreads * 8);
	if (nb > 16384) nb = 16384;
	const auto v = upto_nd(pop.v, pop.nd);
	hipLaunchKernelGGL(k_vel_assert, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, v.a, v.b, v.c, sp.b0, sp.n,
	                   pop.nd, maxVel, errFlag);
	return check_launch("velocity assert");
}

extern "C" long pinc_hip_collide_chunk(void) { return kColChunk; }

// (mix64 of the device code, restated for the host: include/pinc_hip.h)
extern "C" unsigned long long pinc_hip_collide_key(unsigned long long seed, unsigned long long step, int rank, int s) {
	auto mix = [](unsigned long long z) {
		z += 0x9E3779B97F4A7C15ULL;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
		return z ^ (z >> 31);
	};
	return mix(mix(seed ^ mix(step)) ^ mix((unsigned long long)((long)rank * PINC_MAX_SPECIES + s)));
}

extern "C" int pinc_hip_collide(pinc_pop_t pop, int s, double *const v[3], pinc_collide_t c, unsigned long long *counts,
                                void *stream) {
	if (s < 0 || s >= pop.nSpecies || pop.nd < 1 || pop.nd > 3 || !v || !counts)
		return set_error(hipErrorInvalidValue, "collide: bad species, dimensions or null array");
	for (int d = 0; d < pop.nd; d++) {
		if (!v[d]) return set_error(hipErrorInvalidValue, "collide: null velocity array");
		if (!(c.h[d] > 0.0) || !std::isfinite(c.h[d])) return set_error(hipErrorInvalidValue, "collide: h must be > 0");
		if (!std::isfinite(c.drift[d])) return set_error(hipErrorInvalidValue, "collide: drift not finite");
	}
	for (int k = 0; k < 2; k++)
		if (!(c.nu[k] >= 0.0) || !(c.sig[k] >= 0.0) || !std::isfinite(c.nu[k]) || !std::isfinite(c.sig[k]))
			return set_error(hipErrorInvalidValue, "collide: a rate is negative or not finite");
	if (!(c.b >= 0.0 && c.b <= 1.0)) return set_error(hipErrorInvalidValue, "collide: b outside [0, 1]");
	if (!(c.vth >= 0.0) || !std::isfinite(c.vth)) return set_error(hipErrorInvalidValue, "collide: vth negative or not finite");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	const long nb = chunk_blocks(sp.b0, sp.n, kColChunk);
	hipStream_t st = (hipStream_t)stream;
	const auto w = upto_nd(v, pop.nd);
	// cross sections: every particle's neutral is sampled; rates alone: one
	// draw decides and the colliders are processed densely (k_collide)
	const bool eager = c.sig[0] != 0.0 || c.sig[1] != 0.0;
	with_nd(pop.nd, [&](auto ND) {
		if (eager)
			hipLaunchKernelGGL((k_collide<ND, true>), dim3(nb), dim3(kThreads), 0, st, w.a, w.b, w.c, sp.b0, sp.n, c, counts);
		else
			hipLaunchKernelGGL((k_collide<ND, false>), dim3(nb), dim3(kThreads), 0, st, w.a, w.b, w.c, sp.b0, sp.n, c, counts);
	});
	return check_launch("collide");
}

extern "C" long pinc_hip_ionize_chunk(void) { return kIonChunk; }

// the blocks' counts [nb] | their offsets [nb + 1] | scan_ints' work, for the
// nb blocks of n particles at an odd start (chunk_blocks)
extern "C" long pinc_hip_ionize_work(long n) {
	const long nb = ceil_div((n > 0 ? n : 0) + 1, (long)kIonChunk);
	return nb + (nb + 1) + 2 * ceil_div(nb, (long)kScanBlock) + 1;
}

extern "C" unsigned long long pinc_hip_ionize_key(unsigned long long seed, unsigned long long step, int rank, int s) {
	unsigned long long z = pinc_hip_collide_key(seed, step, rank, s) ^ 0x696F6E697365ULL;
	// (mix64, as in pinc_hip_collide_key)
	z += 0x9E3779B97F4A7C15ULL;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}

extern "C" int pinc_hip_ionize(pinc_pop_t pop, int s, pinc_ionize_t c, int *work, long workInts, unsigned long long *res,
                               void *stream) {
	const int t = c.target;
	if (s < 0 || s >= pop.nSpecies || t < 0 || t >= pop.nSpecies || s == t || pop.nSpecies > PINC_MAX_SPECIES)
		return set_error(hipErrorInvalidValue, "ionize: bad projectile or target species");
	if (pop.nd < 1 || pop.nd > 3 || !work || !res)
		return set_error(hipErrorInvalidValue, "ionize: bad dimensions or null array");
	for (int d = 0; d < pop.nd; d++) {
		if (!pop.x[d] || !pop.v[d]) return set_error(hipErrorInvalidValue, "ionize: null particle array");
		if (!(c.h[d] > 0.0) || !std::isfinite(c.h[d])) return set_error(hipErrorInvalidValue, "ionize: h must be > 0");
		if (!std::isfinite(c.drift[d])) return set_error(hipErrorInvalidValue, "ionize: drift not finite");
	}
	if (!(c.nu >= 0.0) || !(c.sig >= 0.0) || !(c.wth >= 0.0) || !(c.vth >= 0.0) || !std::isfinite(c.nu) ||
	    !std::isfinite(c.sig) || !std::isfinite(c.wth) || !std::isfinite(c.vth))
		return set_error(hipErrorInvalidValue, "ionize: a rate, the threshold or vth is negative or not finite");
	for (int q : {s, t})
		if (pop.iStop[q] < pop.iStart[q] || pop.iStop[q] > pop.iStart[q + 1])
			return set_error(hipErrorInvalidValue, "ionize: a species' live range is outside its slots");
	const Span sp = species_span(pop, s);
	if (workInts < pinc_hip_ionize_work(sp.n)) return set_error(hipErrorInvalidValue, "ionize: work too small");
	if (sp.n <= 0) return 0;
	const long nbl = chunk_blocks(sp.b0, sp.n, kIonChunk);
	if (nbl >= (1L << 31)) return set_error(hipErrorInvalidValue, "ionize: too many particles");
	const int nb = (int)nbl;
	const IonSpan is = {sp.b0, sp.n, pop.iStop[s], pop.iStop[t], pop.iStart[s + 1] - pop.iStop[s],
	                    pop.iStart[t + 1] - pop.iStop[t]};
	int *counts = work, *offsets = work + nb;
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, pop.nd), v = upto_nd(pop.v, pop.nd);
	// a cross section: every particle is an entry of the second stage; the
	// rate alone: one draw lists the candidates (k_ionize)
	const bool eager = c.sig != 0.0;
	auto pass = [&](auto ND, auto WRITE) {
		if (eager)
			hipLaunchKernelGGL((k_ionize<ND, true, WRITE>), dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c, is,
			                   c, counts, offsets, nb, res);
		else
			hipLaunchKernelGGL((k_ionize<ND, false, WRITE>), dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c,
			                   is, c, counts, offsets, nb, res);
	};
	with_nd(pop.nd, [&](auto ND) { pass(ND, std::false_type{}); });
	scan_ints(counts, nb, offsets, offsets + (nb + 1), st);
	with_nd(pop.nd, [&](auto ND) { pass(ND, std::true_type{}); });
	return check_launch("ionize");
}

extern "C" int pinc_hip_move_classify(pinc_pop_t pop, int s, int doMove, const double *thr,
                                      unsigned char *flags, int *chunkCount, double maxVel,
                                      int *errFlag, int wrapMask, void *stream) {
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	const int nd = pop.nd;
	const Thr t = make_thr(thr, nd);
	const auto x = upto_nd(pop.x, nd, sp.b0), v = upto_nd(pop.v, nd, sp.b0);
	dim3 grid((unsigned)ceil_div(sp.n, PINC_CHUNK));
	hipStream_t st = (hipStream_t)stream;
	with_nd(nd, [&](auto ND) {
		hipLaunchKernelGGL(k_move_classify<ND>, grid, dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c, sp.n, doMove,
		                   t, flag_center(nd), flags + sp.b0, chunkCount, maxVel, errFlag, wrapMask);
	});
	return check_launch("move_classify");
}

// pinned host words for the extraction's two small reads (a read into
// pageable memory is staged and copied again on the host's wake-up path)
static int *pinned_ints() {
	static int *p = nullptr;
	if (!p && hipHostMalloc((void **)&p, 64 * sizeof(int), hipHostMallocDefault) != hipSuccess) p = nullptr;
	return p;
}

extern "C" int pinc_hip_extract(pinc_pop_t pop, int s, unsigned char *flags, int *chunkCount,
                                int center, int nNeighbors, pinc_extract_ws_t ws, long *nEmig,
                                long *neCount, void *stream) {
	(void)nNeighbors;
	hipStream_t st = (hipStream_t)stream;
	const Span sp = species_span(pop, s);
	const long n = sp.n, sb = sp.b0;
	*nEmig = 0;
	for (int q = 0; q < kMaxNe; q++) neCount[q] = 0;
	if (n <= 0) return 0;
	int nChunks = (int)ceil_div(n, PINC_CHUNK);
	if (nChunks <= 4096 || !ws.scanWork)
		hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, chunkCount, ws.chunkOffset, nChunks);
	else
		scan_ints(chunkCount, nChunks, ws.chunkOffset, ws.scanWork, st);
	int *hp = pinned_ints();
	if (!hp) return set_error(hipErrorOutOfMemory, "extract: pinned host words");
	hipError_t e = hipMemcpyAsync(hp, ws.chunkOffset + nChunks, sizeof(int), hipMemcpyDeviceToHost, st);
	if (e != hipSuccess) return set_error(e, "extract: count readback");
	e = hipStreamSynchronize(st);
	if (e != hipSuccess) return set_error(e, "extract: sync");
	const int E = hp[0];
	*nEmig = E;
	if (E == 0) return check_launch("extract(scan)");
	if (E > ws.cap) return PINC_ERR_CAPACITY;
	hipLaunchKernelGGL(k_extract_a, dim3(nChunks), dim3(kThreads), 0, st, flags + sb, n, center,
	                   ws.chunkOffset, nChunks, ws.tail, ws.holes, ws.order, ws.scratch);
	hipLaunchKernelGGL(k_extract_b, dim3((unsigned)ceil_div(E + 1, 256)), dim3(256), 0, st,
	                   flags + sb, n, (long)E, center, ws.tail, ws.holes, ws.order, ws.scratch);
	int nb = (int)ceil_div(E, kRankChunk);
	hipLaunchKernelGGL(k_rank_hist, dim3(nb), dim3(kThreads), 0, st, flags + sb, ws.order, (long)E,
	                   ws.blockHist);
	hipLaunchKernelGGL(k_hist_scan, dim3(1), dim3(kMaxNe * 32), 0, st, ws.blockHist, nb,
	                   ws.scratch);
	hipLaunchKernelGGL(k_rank_scatter, dim3(nb), dim3(kThreads), 0, st, flags + sb, ws.order,
	                   (long)E, ws.blockHist, ws.scratch, pop, sb, ws.buf, ws.cap, ws.bufNe, center);
	hipLaunchKernelGGL(k_fill_holes, dim3((unsigned)ceil_div(E, 256)), dim3(256), 0, st, pop, sb,
	                   ws.tail, ws.holes, ws.scratch);
	static_assert(kMaxNe <= 64, "pinned words");
	e = hipMemcpyAsync(hp, ws.scratch + 64, kMaxNe * sizeof(int), hipMemcpyDeviceToHost, st);
	if (e != hipSuccess) return set_error(e, "extract: direction counts");
	e = hipStreamSynchronize(st);
	if (e != hipSuccess) return set_error(e, "extract: sync 2");
	for (int q = 0; q < kMaxNe; q++) neCount[q] = hp[q];
	return check_launch("extract");
}

extern "C" int pinc_hip_import(pinc_pop_t pop, int s, long dst, const double *buf, long cap,
                               const unsigned char *bufNe, long first, long n, const int *shiftT,
                               int shiftMask, void *stream) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_import, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
	                   (hipStream_t)stream, pop, pop.iStart[s] + dst, buf, cap, bufNe, first, n,
	                   shiftT[0], shiftT[1], shiftT[2], shiftMask);
	return check_launch("import");
}

extern "C" int pinc_hip_pack(const double *buf, long cap, const unsigned char *bufNe, long first, long n,
                             int nd, double *out, void *stream) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_pack, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, buf, cap,
	                   bufNe, first, n, nd, out);
	return check_launch("pack");
}

extern "C" int pinc_hip_import_rec(pinc_pop_t pop, int s, long dst, const double *rec, long n,
                                   const int *shiftT, void *stream) {
	if (n <= 0) return 0;
	hipLaunchKernelGGL(k_import_rec, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, pop,
	                   pop.iStart[s] + dst, rec, n, shiftT[0], shiftT[1], shiftT[2]);
	return check_launch("import_rec");
}

extern "C" int pinc_hip_deposit(pinc_pop_t pop, int s, pinc_geom_t g, double *rho, void *stream) {
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = chunk_blocks(sp.b0, sp.n, kDepChunk);
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL((k_deposit_tiled<ND, ND == 3>), dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, sp.b0, sp.n,
		                   g, rho);
	});
	return check_launch("deposit");
}

extern "C" int pinc_hip_moments(pinc_pop_t pop, int s, pinc_geom_t g, const double *const v[3], double *momSlab,
                                void *stream) {
	if (g.nd < 1 || g.nd > 3 || s < 0 || s >= PINC_MAX_SPECIES || !v || !momSlab)
		return set_error(hipErrorInvalidValue, "moments: bad species, dimensions or null array");
	for (int d = 0; d < g.nd; d++)
		if (!pop.x[d] || !v[d]) return set_error(hipErrorInvalidValue, "moments: null particle array");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nb = chunk_blocks(sp.b0, sp.n, kMomChunk);
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd);
	const auto w = upto_nd(v, g.nd);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL((k_moments<ND>), dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, w.a, w.b, w.c, sp.b0, sp.n, g,
		                   momSlab);
	});
	return check_launch("moments");
}

extern "C" long pinc_hip_phase_lds_bins(void) { return kPhLds; }

extern "C" int pinc_hip_phase_hist(pinc_pop_t pop, int s, const double *const v[3], pinc_phase_t spec,
                                   unsigned long long *hist, unsigned long long *outside, void *stream) {
	if (pop.nd < 1 || pop.nd > 3 || s < 0 || s >= PINC_MAX_SPECIES || !v || !hist || !outside)
		return set_error(hipErrorInvalidValue, "phase_hist: bad species, dimensions or null array");
	const int na = spec.axis[1] == PINC_PS_NONE ? 1 : 2;
	const double *c[2] = {nullptr, nullptr};
	for (int a = 0; a < na; a++) {
		const int ax = spec.axis[a];
		if (ax < PINC_PS_X || ax > PINC_PS_VZ) return set_error(hipErrorInvalidValue, "phase_hist: axis is no PINC_PS_*");
		if (ax % 3 >= pop.nd) return set_error(hipErrorInvalidValue, "phase_hist: axis beyond the population's dimensions");
		c[a] = ax < PINC_PS_VX ? pop.x[ax] : v[ax - PINC_PS_VX];
		if (!c[a]) return set_error(hipErrorInvalidValue, "phase_hist: null particle array");
		if (spec.nbins[a] < 1) return set_error(hipErrorInvalidValue, "phase_hist: nbins < 1");
	}
	if (na == 1 && spec.nbins[1] != 1) return set_error(hipErrorInvalidValue, "phase_hist: nbins[1] != 1 without a second axis");
	if ((long)spec.nbins[0] * spec.nbins[1] > (1L << 24))
		return set_error(hipErrorInvalidValue, "phase_hist: more than 2^24 bins");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	const long nb = chunk_blocks(sp.b0, sp.n, kPhChunk);
	hipStream_t st = (hipStream_t)stream;
	if (na == 1)
		hipLaunchKernelGGL((k_phase_hist<1>), dim3(nb), dim3(kThreads), 0, st, c[0], c[1], sp.b0, sp.n, spec, hist, outside);
	else
		hipLaunchKernelGGL((k_phase_hist<2>), dim3(nb), dim3(kThreads), 0, st, c[0], c[1], sp.b0, sp.n, spec, hist, outside);
	return check_launch("phase_hist");
}

extern "C" int pinc_hip_field_chain_all(const double *E, double *Es, long n, const double *qm, const double *mq,
                                        double pre, int nSpecies, void *stream) {
	if (n > 0 && (!E || !Es || !qm || !mq)) return set_error(hipErrorInvalidValue, "field_chain_all: null array");
	if (nSpecies < 1 || nSpecies > PINC_MAX_SPECIES)
		return set_error(hipErrorInvalidValue, "field_chain_all: species count");
	if (n <= 0) return 0;
	long nb = ceil_div(n, (long)kThreads * 4);
	if (nb > 8192) nb = 8192;
	hipLaunchKernelGGL(k_field_chain_all, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, E, Es, n, qm, mq, pre,
	                   nSpecies);
	return check_launch("field chain (all species)");
}

extern "C" int pinc_hip_field_chain(const double *E, double *Es, long n, const double *qm,
                                    const double *mq, double pre, int s, void *stream) {
	if (n > 0 && (!E || !Es || !qm || !mq)) return set_error(hipErrorInvalidValue, "field_chain: null array");
	if (n <= 0) return 0;
	long nb = ceil_div(n, (long)kThreads * 4);
	if (nb > 8192) nb = 8192;
	hipLaunchKernelGGL(k_field_chain, dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, E, Es, n, qm, mq, pre, s);
	return check_launch("field chain");
}

// k_accel's blocks take kAccChunk slots from the even index at or below b0
// (chunk_blocks), so that its paired loads stay 16-byte aligned
extern "C" int pinc_hip_accelerate(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es,
                                   double *kePartial, int *nBlocks, void *stream) {
	const Span sp = species_span(pop, s);
	*nBlocks = 0;
	if (sp.n <= 0) return 0;
	if (!Es) return set_error(hipErrorInvalidValue, "accelerate: null E");
	long nb = chunk_blocks(sp.b0, sp.n, kAccChunk);
	*nBlocks = (int)nb;
	hipStream_t st = (hipStream_t)stream;
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL((k_accel<ND, ND == 3, true>), dim3(nb), dim3(kThreads), 0, st, pop.x[0], pop.x[1], pop.x[2],
		                   pop.v[0], pop.v[1], pop.v[2], sp.b0, sp.n, g, Es, kePartial);
	});
	return check_launch("accelerate");
}

extern "C" int pinc_hip_boris(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, const double *T,
                              const double *S, double *kePartial, int *nBlocks, void *stream) {
	const Span sp = species_span(pop, s);
	*nBlocks = 0;
	if (g.nd != 3 || pop.nd != 3) return set_error(hipErrorInvalidValue, "boris: 3-D only (puBoris3D1)");
	if (sp.n <= 0) return 0;
	long nb = chunk_blocks(sp.b0, sp.n, kAccChunk);
	*nBlocks = (int)nb;
	BorisRot rot;
	for (int q = 0; q < 3; q++) {
		rot.T[q] = T[q];
		rot.S[q] = S[q];
	}
	hipLaunchKernelGGL((k_accel<3, true, true, true>), dim3(nb), dim3(kThreads), 0, (hipStream_t)stream, pop.x[0],
	                   pop.x[1], pop.x[2], pop.v[0], pop.v[1], pop.v[2], sp.b0, sp.n, g, Es, kePartial, rot);
	return check_launch("boris");
}

extern "C" int pinc_hip_init_species(pinc_pop_t pop, int s, pinc_geom_t g, long nGlobal,
                                     double latticeStep, const int *subdomain,
                                     const int *nSubdomains, const int *offset, const double *amp,
                                     const double *mode, int perturb, int maxwell, double drift,
                                     double vth, unsigned long long seed, long *nOut,
                                     void *stream) {
	hipStream_t st = (hipStream_t)stream;
	if (nGlobal <= 0) {
		*nOut = 0;
		return 0;
	}
	LatticeArgs a;
	a.nd = g.nd;
	for (int d = 0; d < 3; d++) {
		a.L[d] = d < g.nd ? g.T[d] : 1;
		a.sub[d] = d < g.nd ? subdomain[d] : 0;
		a.off[d] = d < g.nd ? offset[d] : 0;
		int tsd = d < g.nd ? (g.T[d] / nSubdomains[d]) : 1;
		a.posToSub[d] = (double)1 / tsd;
		a.amp[d] = d < g.nd ? amp[d] : 0;
		a.mode[d] = d < g.nd ? mode[d] : 0;
	}
	a.l = latticeStep;
	a.perturb = perturb;
	a.maxwell = maxwell;
	a.drift = drift;
	a.vth = vth;
	a.seed = seed;
	a.species = s;
	long nChunks = ceil_div(nGlobal, PINC_CHUNK);
	int *cnt = nullptr, *off = nullptr;
	hipError_t e = hipMallocAsync((void **)&cnt, (nChunks + 1) * sizeof(int), st);
	if (e != hipSuccess) return set_error(e, "init: alloc");
	e = hipMallocAsync((void **)&off, (nChunks + 1) * sizeof(int), st);
	if (e != hipSuccess) return set_error(e, "init: alloc");
	hipLaunchKernelGGL(k_lattice_count, dim3((unsigned)nChunks), dim3(kThreads), 0, st, a, nGlobal, cnt);
	hipLaunchKernelGGL(k_scan_single, dim3(1), dim3(1024), 0, st, cnt, off, (int)nChunks);
	int total = 0;
	e = hipMemcpyAsync(&total, off + nChunks, sizeof(int), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess) e = hipStreamSynchronize(st);
	if (e != hipSuccess) return set_error(e, "init: count readback");
	long capS = pop.iStart[s + 1] - pop.iStart[s];
	if (total > capS) {
		(void)hipFreeAsync(cnt, st);
		(void)hipFreeAsync(off, st);
		return set_error(hipErrorOutOfMemory, "init: species capacity too small");
	}
	hipLaunchKernelGGL(k_lattice_write, dim3((unsigned)nChunks), dim3(kThreads), 0, st, a, nGlobal,
	                   off, pop, pop.iStart[s]);
	(void)hipFreeAsync(cnt, st);
	(void)hipFreeAsync(off, st);
	*nOut = total;
	return check_launch("init_species");
}

// The sorting push reserves its output per brick of
// tw^(nd-1) cells (tw x tw x 1 in 3-D, one block's worth at C4's 64 ppc)
// instead of per cell: a few tens of runs per block instead of about a
// hundred short scattered ones once the input order has decayed; inside a
// brick run the block's particles stay grouped by cell.  (Tried: bricks
// ordered along the slab dimension fastest, so that consecutive bricks are
// neighbours -- the plain pushes got slower, 25 -> 31 ms per ion launch at
// C4: the concurrently running blocks then touch scattered grid rows.)

static TileGeo make_tile_geo(pinc_geom_t g, int tileWidth, long *nKeys) {
	TileGeo tg;
	long nt = 1, cpt = 1;
	tg.tw = tileWidth;
	int lw = 0;
	while ((1 << lw) < tileWidth) lw++;
	const bool brick = (1 << lw) == tileWidth;
	for (int d = 0; d < 3; d++) {
		int T = d < g.nd ? (d == g.nd - 1 ? g.nloc : g.T[d]) : 1;
		tg.cmax[d] = T + 1;
		tg.nt[d] = d < g.nd ? (T + 1) / tileWidth + 1 : 1;
		tg.bs[d] = brick && d < g.nd - 1 ? lw : 0;
		nt *= tg.nt[d];
		if (d < g.nd) cpt *= tileWidth;
	}
	*nKeys = nt * cpt;
	return tg;
}

extern "C" int pinc_hip_sort_tiles(pinc_pop_t pop, pinc_pop_t out, int s, pinc_geom_t g, int tileWidth,
                                   int *work, long workCap, long *nKeysOut, void *stream) {
	long nk = 0;
	TileGeo tg = make_tile_geo(g, tileWidth, &nk);
	long nsb = ceil_div(nk, (long)kScanBlock);
	*nKeysOut = nk;
	// work: counts[nk+1] | offsets[nk+1] | scan_ints' work
	long need = 2 * (nk + 1) + 2 * nsb + 1;
	if (need > workCap || nk > 2147483647L) return set_error(hipErrorInvalidValue, "sort_tiles: work buffer too small");
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	if (sp.n > 2147483647L) return set_error(hipErrorInvalidValue, "sort_tiles: species too large for int slots");
	hipStream_t st = (hipStream_t)stream;
	int *counts = work, *offs = work + (nk + 1);
	hipError_t e = hipMemsetAsync(counts, 0, (nk + 1) * sizeof(int), st);
	if (e != hipSuccess) return set_error(e, "sort_tiles: memset");
	long nb = ceil_div(sp.n, (long)kThreads);
	if (nb > 65536L * 8) nb = 65536L * 8;
	const auto x = upto_nd(pop.x, g.nd, sp.b0);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_sort_count<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, sp.n, tg, counts);
	});
	scan_ints(counts, nk, offs, offs + (nk + 1), st);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_sort_scatter<ND>, dim3(nb), dim3(kThreads), 0, st, pop, out, sp.b0, sp.n, tg, offs);
	});
	return check_launch("sort_tiles");
}

extern "C" int pinc_hip_deposit_cells(pinc_pop_t pop, int s, pinc_geom_t g, int tileWidth, const int *offs,
                                      long nCell, double *rho, void *stream) {
	const Span sp = species_span(pop, s);
	if (sp.n <= 0) return 0;
	long nKeys = 0;
	TileGeo tg = make_tile_geo(g, tileWidth, &nKeys);
	if (nCell > sp.n) nCell = sp.n;
	hipStream_t st = (hipStream_t)stream;
	const auto x = upto_nd(pop.x, g.nd, sp.b0);
	unsigned nb = (unsigned)ceil_div(nKeys, (long)kThreads);
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL((k_deposit_cells<ND, ND == 3>), dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, nCell, offs,
		                   nKeys, tg, g, rho);
	});
	int rc = check_launch("deposit_cells");
	if (rc || nCell >= sp.n) return rc;
	// particles appended since the sort (immigrants): generic deposit
	pinc_pop_t tail = pop;
	tail.iStart[s] = sp.b0 + nCell;
	return pinc_hip_deposit(tail, s, g, rho, stream);
}

extern "C" int pinc_hip_push(pinc_pop_t pop, int s, pinc_geom_t g, const pinc_push_t *args, int *nBlocks,
                             void *stream) {
	const Span sp = species_span(pop, s);
	*nBlocks = 0;
	if (sp.n <= 0) return 0;
	const long b0 = sp.b0;
	int nd = pop.nd;
	if (nd != g.nd) return set_error(hipErrorInvalidValue, "push: population and grid dimensions differ");
	const bool sort = args->cursor != nullptr;
	if (sort && sp.n > 2147483647L) return set_error(hipErrorInvalidValue, "push: species too large for int slots");
	long nodes = 1;
	for (int d = 0; d < nd; d++) nodes *= (d == nd - 1) ? (long)g.nloc + 2 : (long)g.T[d];
	if (nodes * nd >= 2147483647L) return set_error(hipErrorInvalidValue, "push: grid too large for 32-bit offsets");
	PushArgs a;
	for (int d = 0; d < 3; d++) {
		a.xi[d] = d < nd ? pop.x[d] + b0 : nullptr;
		a.xo[d] = d < nd ? args->xout[d] + b0 : nullptr;
		a.vi[d] = d < nd ? pop.v[d] + b0 : nullptr;
		a.vo[d] = d < nd ? args->vout[d] + b0 : nullptr;
	}
	a.thr = make_thr(args->thr, nd);
	a.n = sp.n;
	a.g = g;
	a.Es = args->Es;
	a.rho = args->rhoS;
	a.center = flag_center(nd);
	a.wrapMask = args->wrapMask;
	a.maxVel = args->maxVel;
	a.flags = args->flags + b0;
	a.chunkCount = args->chunkCount;
	a.err = args->errFlag;
	a.kePartial = args->kePartial;
	long nKeys = 0;
	a.tg = make_tile_geo(g, args->tileWidth > 0 ? args->tileWidth : 1, &nKeys);
	a.cursor = args->cursor;
	a.cntNext = args->cntNext;
	a.moved = args->moved;
	a.spread = args->spread;
	a.tstamp = args->tstamp;
	a.diag = args->diag;
	a.emigTotal = args->emigTotal;
	a.flagsSparse = args->flagsSparse;
	a.objIn = args->objInside;
	a.objSy = args->objSy;
	a.objSz = args->objSz;
	a.objN = args->objNodes;
	a.objCount = args->objCount;
	for (int d = 0; d < 3; d++) {
		a.objLo[d] = args->objLo[d];
		a.objExt[d] = args->objHi[d] - args->objLo[d];
	}
	if (a.objIn && !a.objCount) return set_error(hipErrorInvalidValue, "push: objInside without objCount");
	if (a.objIn && (nd != 3 || a.objN > 2147483647L)) return set_error(hipErrorInvalidValue, "push: objects are 3-D");
	for (int d = 0; a.objIn && d < 3; d++)
		if (a.objExt[d] >= 0 && (a.objLo[d] < 0 || (long)a.objLo[d] + a.objExt[d] >= (d == 0 ? a.objSy : d == 1 ? a.objSz / a.objSy
		                                                                                             : a.objN / a.objSz)))
			return set_error(hipErrorInvalidValue, "push: object box outside the node table");
	unsigned nb = (unsigned)ceil_div(sp.n, kPushChunk);
	*nBlocks = (int)nb;
	hipStream_t st = (hipStream_t)stream;
	const bool kick = args->kick != 0;
	if (kick && !args->Es) return set_error(hipErrorInvalidValue, "push: kick without E");
	// a sorting push never counts (its brick counters use the count's LDS)
	if (sort) a.cntNext = nullptr;
	auto launch = [&](auto ND, auto OBJ) {
		constexpr bool V3D = ND == 3;
		if (kick && sort) hipLaunchKernelGGL((k_push<ND, V3D, true, true, OBJ>), dim3(nb), dim3(kPushThreads), 0, st, a);
		else if (kick) hipLaunchKernelGGL((k_push<ND, V3D, true, false, OBJ>), dim3(nb), dim3(kPushThreads), 0, st, a);
		else if (sort) hipLaunchKernelGGL((k_push<ND, V3D, false, true, OBJ>), dim3(nb), dim3(kPushThreads), 0, st, a);
		else hipLaunchKernelGGL((k_push<ND, V3D, false, false, OBJ>), dim3(nb), dim3(kPushThreads), 0, st, a);
	};
	// (the object test exists in the 3-D instances only)
	with_nd(nd, [&](auto ND) {
		if constexpr (ND == 3) {
			if (a.objIn) return launch(ND, std::true_type{});
		}
		launch(ND, std::false_type{});
	});
	return check_launch("push");
}

extern "C" long pinc_hip_tile_keys(pinc_geom_t g, int tileWidth) {
	long nk = 0;
	(void)make_tile_geo(g, tileWidth, &nk);
	return nk;
}

extern "C" int pinc_hip_count_keys(pinc_pop_t pop, int s, long first, pinc_geom_t g, int tileWidth, int *counts,
                                   void *stream) {
	long b0 = pop.iStart[s] + first;
	long n = pop.iStop[s] - b0;
	if (n <= 0) return 0;
	long nk = 0;
	TileGeo tg = make_tile_geo(g, tileWidth, &nk);
	long nb = ceil_div(n, (long)kThreads);
	if (nb > 65536L * 8) nb = 65536L * 8;
	const auto x = upto_nd(pop.x, g.nd, b0), v = upto_nd(pop.v, g.nd, b0);
	hipStream_t st = (hipStream_t)stream;
	with_nd(g.nd, [&](auto ND) {
		hipLaunchKernelGGL(k_count_bricks<ND>, dim3(nb), dim3(kThreads), 0, st, x.a, x.b, x.c, v.a, v.b, v.c, n, tg,
		                   counts);
	});
	return check_launch("count_keys");
}

extern "C" int pinc_hip_scan_keys(const int *counts, long nKeys, int *offsets, int *work, void *stream) {
	if (ceil_div(nKeys, (long)kScanBlock) > 1024L * 1024L)
		return set_error(hipErrorInvalidValue, "scan_keys: too many keys");
	scan_ints(counts, nKeys, offsets, work, (hipStream_t)stream);
	return check_launch("scan_keys");
}

extern "C" int pinc_hip_rho_combine(double *rho, const double *const *acc, const double *charge, int ns, long n,
                                    void *stream) {
	if (ns < 1 || ns > PINC_MAX_SPECIES) return set_error(hipErrorInvalidValue, "rho_combine: species");
	if (n <= 0) return 0;
	CombineArgs c;
	c.ns = ns;
	for (int s = 0; s < PINC_MAX_SPECIES; s++) {
		c.acc[s] = s < ns ? acc[s] : nullptr;
		c.q[s] = s < ns ? charge[s] : 1.0;
	}
	long nb = ceil_div(n, (long)kThreads * 4);
	if (nb > 8192) nb = 8192;
	hipLaunchKernelGGL(k_rho_combine, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, rho, c, n);
	return check_launch("rho_combine");
}
