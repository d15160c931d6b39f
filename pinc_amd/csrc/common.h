// common.h -- shared device helpers for the PINC MI355X kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "pinc_hip.h"

#define PINC_WAVE 64

namespace pinc {

// error bookkeeping shared by all translation units (runtime.hip)
int set_error(hipError_t e, const char *where);
int check_launch(const char *where);

// ---- host-side launch helpers of the C ABI ----
// f(std::integral_constant<int, ND>) for the kernel instance of nd
// dimensions: 3, 2, and the 1-D instance for anything else
template <class F>
inline void with_nd(int nd, F &&f) {
	if (nd == 3) f(std::integral_constant<int, 3>{});
	else if (nd == 2) f(std::integral_constant<int, 2>{});
	else f(std::integral_constant<int, 1>{});
}

// live particles of species s: indices b0 .. b0 + n - 1
struct Span {
	long b0, n;
};
inline Span species_span(const pinc_pop_t &pop, int s) { return {pop.iStart[s], pop.iStop[s] - pop.iStart[s]}; }

// the per-dimension pointers p[0..2] as kernel arguments: null above nd,
// the others advanced by b0
template <class T>
struct Ptr3 {
	T *a, *b, *c;
};
template <class T>
inline Ptr3<T> upto_nd(T *const *p, int nd, long b0 = 0) {
	return {p[0] + b0, nd > 1 ? p[1] + b0 : nullptr, nd > 2 ? p[2] + b0 : nullptr};
}

// storage index of a padded coordinate p (0..T+1) in a periodic dimension
// stored without ghosts (grid.c halo semantics: ghost 0 == T, T+1 == 1)
__device__ __forceinline__ int wrap_pad(int p, int T) {
	int s = p - 1;
	s = (s < 0) ? s + T : s;
	s = (s >= T) ? s - T : s;
	return s;
}

// periodic neighbour in a ghost-free dimension
__device__ __forceinline__ int wrap(int i, int T) {
	return (i < 0) ? i + T : ((i >= T) ? i - T : i);
}

// Grid-stride walk of the point stencils (residual, norm, restriction,
// prolongation, E = -grad phi).  With a multiple of 8 blocks, the 8 XCDs
// (block b on XCD b % 8) take contiguous eighths of [0, n) and each XCD's
// blocks sweep theirs in order, so the rows and planes a point's stencil
// reads around it are read by the same XCD close in time (one L2), instead
// of by the XCDs of the blocks of the neighbouring rows.  Placement only:
// the same points, the same arithmetic.  Otherwise the plain grid stride.
struct Walk {
	long g0, g1, step;
};
__device__ __forceinline__ Walk point_walk(long n) {
	const long nt = blockDim.x;
	if ((gridDim.x & 7u) == 0) {
		const unsigned x = blockIdx.x & 7u, j = blockIdx.x >> 3, perXcd = gridDim.x >> 3;
		const long span = ((n + 8 * nt - 1) / (8 * nt)) * nt;  // an eighth, whole blocks
		const long b0 = (long)x * span;
		return {b0 + (long)j * nt + threadIdx.x, min(n, b0 + span), (long)perXcd * nt};
	}
	return {(long)blockIdx.x * nt + threadIdx.x, n, (long)gridDim.x * nt};
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		T u = __shfl_up(v, o, 64);
		if (lane >= o) v += u;
	}
	return v;
}

// deterministic block sum (fixed shape: blockDim multiple of 64, <=1024)
__device__ __forceinline__ double block_sum(double v, double *lds) {
	v = wave_sum(v);
	int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (lane == 0) lds[w] = v;
	__syncthreads();
	double r = 0.;
	if (threadIdx.x == 0) {
		int nw = blockDim.x >> 6;
		for (int i = 0; i < nw; i++) r += lds[i];
	}
	__syncthreads();
	return r;  // valid in thread 0
}

}  // namespace pinc
