/*
 * pinc_hip.h -- C ABI of the MI355X kernel library (libpinc_hip.so).
 *
 * Plain C: pointers, sizes and small POD structs only; no HIP or torch types
 * cross this boundary (streams are opaque void*).  Every entry point returns
 * 0 on success or a nonzero HIP/RCCL error code; pinc_hip_error_string()
 * describes the last failure.  The host operator surface (include/pinc.h)
 * is built on these calls; each entry cites the reference loop it replaces.
 *
 * Device data layout (DESIGN.md "Layout"):
 *   particles  SoA per component, species s in [iStart[s], iStart[s+1]) with
 *              live particles [iStart[s], iStop[s]) -- the reference's
 *              Population ranges (core.h:72-86) with x,y,z,vx,vy,vz split.
 *              Positions are in the reference's local frame (true nodes at
 *              1..T, ghosts 0 and T+1).
 *   slab grid  the decomposed (last) dimension keeps its two ghost planes,
 *              the other dimensions are periodic and stored without ghosts:
 *              3-D [nloc+2][Ty][Tx], 2-D [nloc+2][Tx], 1-D [nloc+2].
 *              Vector grids (E) hold 3 doubles per node (xyz, value-major as
 *              grid.c:413-500).
 *   global     the whole periodic domain without ghosts [Tz][Ty][Tx] (MG,
 *              spectral); with one rank it aliases the slab's true planes.
 */
#ifndef PINC_HIP_H
#define PINC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PINC_MAX_SPECIES 8
#define PINC_MAX_LEVELS 12

/* geometry of one rank's slab; dims ordered x,y,z; slab dim = nd-1 */
typedef struct {
	int nd;        /* 1..3 */
	int T[3];      /* global true size per dim (1 for unused dims) */
	int nloc;      /* true cells of this rank along the slab dimension */
	int off;       /* first true cell of this rank along the slab dim */
	int nranks;    /* slabs along the slab dimension */
	int literal;   /* main.c's double rho FROMHALO (literal loop): 1 = deposits on
	                  periodic ghost nodes of the non-slab dims count twice per
	                  ghost coordinate; 2 = only the weight a plain deposit
	                  misses for a second fold, (2^g - 1) per weight, doubled on
	                  slab ghost planes (the second fold adds them once more) */
} pinc_geom_t;

/* a population on the device (by value; pointers are device pointers) */
typedef struct {
	double *x[3];
	double *v[3];
	int nSpecies;
	int nd;
	long iStart[PINC_MAX_SPECIES + 1];
	long iStop[PINC_MAX_SPECIES];
} pinc_pop_t;

/* ------------------------------------------------------------ runtime -- */
const char *pinc_hip_error_string(void);
int pinc_hip_set_device(int dev);
int pinc_hip_device_count(int *n);
int pinc_hip_stream_create(void **stream);
/* Stream capture of a fixed launch sequence into a graph (MG V-cycle replay;
 * replaces the reference's per-call dispatch, no reference counterpart):
 * begin on a non-default stream, end -> instantiated executable, launch on a
 * stream, destroy. */
int pinc_hip_capture_begin(void *stream);
int pinc_hip_capture_end(void *stream, void **exec);
int pinc_hip_graph_launch(void *exec, void *stream);
int pinc_hip_graph_destroy(void *exec);
int pinc_hip_stream_destroy(void *stream);
int pinc_hip_stream_sync(void *stream);
int pinc_hip_device_sync(void);
int pinc_hip_malloc(void **ptr, unsigned long bytes);
int pinc_hip_free(void *ptr);
int pinc_hip_memset(void *ptr, int value, unsigned long bytes, void *stream);
int pinc_hip_h2d(void *dst, const void *src, unsigned long bytes, void *stream);
int pinc_hip_d2h(void *dst, const void *src, unsigned long bytes, void *stream);
int pinc_hip_d2d(void *dst, const void *src, unsigned long bytes, void *stream);
/* asynchronous device-to-host copy (dst: pinned memory from
 * pinc_hip_host_alloc), complete once an event recorded after it is
 * (pinc_hip_event_sync): the host keeps enqueueing work meanwhile (the
 * multigrid's per-cycle norm, pinc_mg.c) */
int pinc_hip_d2h_async(void *dst, const void *src, unsigned long bytes, void *stream);
int pinc_hip_host_alloc(void **ptr, unsigned long bytes);
int pinc_hip_host_free(void *ptr);
int pinc_hip_event_sync(void *ev);
/* events for per-phase device timing (replaces Timer, aux.c:48-85) */
int pinc_hip_event_create(void **ev);
int pinc_hip_event_destroy(void *ev);
int pinc_hip_event_record(void *ev, void *stream);
int pinc_hip_event_elapsed(float *ms, void *start, void *stop);
int pinc_hip_mem_info(unsigned long *freeBytes, unsigned long *totalBytes);

/* --------------------------------------------------------- particles -- */
/* puMove (pusher.c:86-119, as compiled: pos += vel) fused with the
 * neighbour classification of puExtractEmigrants3D/ND (pusher.c:782-910):
 * flags[i] = ne in 0..3^nd-1, center = stays.  chunkCount[b] = emigrants of
 * chunk b (PINC_CHUNK particles).  If doMove is 0 only classifies.
 * thr = [lower(nd), upper(nd), size-1 (nd)] as MpiInfo.thresholds.
 * wrapMask bit d (tiled layout only): a crossing in dimension d is applied in
 * place with the import's periodic shift and does not count as emigration;
 * 0 reproduces the reference exactly. */
#define PINC_CHUNK 2048
int pinc_hip_move_classify(pinc_pop_t pop, int s, int doMove, const double *thr,
                           unsigned char *flags, int *chunkCount, double maxVel,
                           int *errFlag, int wrapMask, void *stream);

/* Fused push of species s: optionally puAcc's kick
 * (kick=1: gather from Es as pinc_hip_accelerate, v += dv, KE partials of
 * blocks of PINC_CHUNK/2 particles in kePartial, *nBlocks of them), then
 * puMove's drift, the classification of pinc_hip_move_classify (flags,
 * chunkCount -- zeroed by the caller -- errFlag, wrapMask) and the CIC
 * deposit (puDistr3D1/ND1 weights) of every particle that stays into the
 * species accumulator rhoS (slab layout, not zeroed here).  With the slab
 * dimension wrapped in place (wrapMask bit nd-1) a block that straddles that
 * boundary deposits at the periodic images of its cells, so a node's charge
 * may lie on ghost plane 0 or on true plane nloc (nloc+1 or 1): only the sum
 * after the halo fold (pinc_hip_fold_self) is defined, and E's ghost planes
 * must be the periodic copies (plane 0 = plane nloc, plane nloc+1 = plane 1).
 *   cursor == NULL: particle i stays at i; new positions go to xout (may be
 *     pop.x), velocities to vout (may be pop.v).
 *   cursor != NULL (tiled layout, sorted output): particle i goes to slot
 *     cursor[key(x_i)]++ (cursor = exclusive scan of the key counts of the
 *     current positions, pinc_hip_count_keys + pinc_hip_scan_keys), its
 *     moved state to xout/vout at that slot (must not alias pop), flags at
 *     that slot; chunkCount counts emigrants per destination chunk.
 *     key(x_i) is the key pinc_hip_count_keys counts: that of the brick
 *     holding the cell of x_i + v_i, both as the push reads them (before
 *     its kick and drift), clamped to the grid.
 *     Otherwise (cursor == NULL) the keys of the moved particles that stay
 *     are counted into cntNext if set (zeroed by the caller); a sorting
 *     push does not count. */
typedef struct {
	double *xout[3];
	double *vout[3];
	int kick;
	const double *Es;
	double *rhoS;
	const double *thr;
	unsigned char *flags;
	int *chunkCount;
	double maxVel;
	int *errFlag;
	int wrapMask;
	double *kePartial;
	int tileWidth;
	int *cursor;
	int *cntNext;
	unsigned long long *moved; /* if set: += particles that stay and changed cell */
	unsigned long long *spread; /* if set: += each block's input cell-box volume (cells spanned by its
	                             * items, periodic images nearest its first item) */
	unsigned long long *tstamp; /* if set: 8 phase timestamps per block (diagnostics) */
	unsigned long long *diag;   /* if set: [0] += items of a sorting push given a global slot one by
	                             * one (outside its LDS boxes; diagnostics) */
	/* immersed objects (fused collection, oCollectObjectCharge's test at
	 * object.c:489-494 on the moved position): if objInside is set, a
	 * particle that stays and whose cell's lower node has an object id > 0
	 * in objInside (padded local nodes, strides 1, objSy, objSz; objNodes
	 * nodes) is flagged PINC_NE_SINK instead of deposited, and counted in
	 * objCount[id - 1] */
	const unsigned char *objInside;
	long objSy, objSz, objNodes;
	int *objCount;
	int objLo[3], objHi[3];   /* bounding box (padded node coordinates, inclusive)
	                             of the nodes with an id: only cells there are looked up */
	unsigned long long *emigTotal; /* if set: += the particles flagged to leave (every flag but the
	                                  centre: emigrants, collected, outside the frame) */
	int flagsSparse;  /* 1: write only the flags that are not the centre (every other flag of the
	                     species' range must already be the centre: pinc_hip_extract puts the
	                     extracted particles' flags back to it); 0: write every live particle's flag */
} pinc_push_t;
int pinc_hip_push(pinc_pop_t pop, int s, pinc_geom_t g, const pinc_push_t *args, int *nBlocks, void *stream);
/* number of sort keys (cells incl. the wrap layer) of the tiled layout */
long pinc_hip_tile_keys(pinc_geom_t g, int tileWidth);
/* counts[key(x_i)] += 1 for particles iStart[s]+first .. iStop[s]-1 */
int pinc_hip_count_keys(pinc_pop_t pop, int s, long first, pinc_geom_t g, int tileWidth, int *counts, void *stream);
/* exclusive scan of nKeys counts (offsets[nKeys] = total); work holds
 * 2*ceil(nKeys/4096)+1 ints */
int pinc_hip_scan_keys(const int *counts, long nKeys, int *offsets, int *work, void *stream);
/* puBoris3D1KE (pusher.c:433-483; rotation parameters pusher.c:485-505) with
 * the reference's indexing defect corrected: per particle a half kick from
 * Es (E as rescaled for species s), v' = v + v x T, v += v' x S (addCross
 * order), KE partial of v^2, half kick.  T, S: host pointers to species s's
 * three components each.  3-D only. */
int pinc_hip_boris(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, const double *T, const double *S,
                   double *kePartial, int *nBlocks, void *stream);
/* rho = the reference's per-species chain (gZero; gMul(1/q_s); add species
 * s; gMul(q_s); pusher.c:512-572) applied to per-species sums acc[s], over
 * n slab elements */
int pinc_hip_rho_combine(double *rho, const double *const *acc, const double *charge, int ns, long n,
                         void *stream);

/* Tiled layout (population:layout = tiled, not in the reference): counting
 * sort of species s by cell, cells grouped in tiles of tileWidth^nd, from
 * pop into out (same ranges); the caller swaps the two.  nKeysOut returns
 * the number of keys K (cells incl. the wrap layer); work must hold
 * 2*(K+1) + 2*ceil(K/4096) + 1 ints (workCap), else an error is returned
 * with nKeysOut set.  Order within a cell is arbitrary. */
int pinc_hip_sort_tiles(pinc_pop_t pop, pinc_pop_t out, int s, pinc_geom_t g, int tileWidth,
                        int *work, long workCap, long *nKeysOut, void *stream);
/* Cell ranges of the last sort: work + (K+1) holds, after pinc_hip_sort_tiles,
 * the exclusive end of each cell's particle range.  puDistr over those
 * ranges: one thread per cell sums its particles' weights in registers;
 * particles that left their cell since the sort, and particles at index
 * >= nCell (appended since), are deposited individually. */
int pinc_hip_deposit_cells(pinc_pop_t pop, int s, pinc_geom_t g, int tileWidth, const int *cellEnds,
                           long nCell, double *rhoSlab, void *stream);

/* Emigrant extraction with the reference's back-fill order (pusher.c:
 * 782-855): survivors fill holes from the tail, emigrants are listed in the
 * exact order the serial loop extracts them, then stably bucketed by
 * direction.  Work arrays: see DESIGN.md "Migration".  Outputs:
 *   buf   (6 doubles per emigrant, SoA blocks of cap entries: x,y,z,vx,vy,vz)
 *   bufNe direction of each buffered emigrant
 *   neCount[PINC_NE_CODES] emigrants per direction (species s), then the
 *         particles a fused push collected into objects (PINC_NE_SINK)
 * Returns the number of emigrants in *nEmig.  Compacts species s in place
 * (iStop[s] decreases by *nEmig on the host side). */
typedef struct {
	int *chunkOffset;   /* nChunks+1 */
	int *scanWork;      /* 2*ceil(nChunks/4096)+1 (multi-block scan of the chunk counts) */
	int *tail;          /* >= nEmig+1 */
	int *holes;         /* >= nEmig+1 */
	int *order;         /* >= nEmig   */
	int *blockHist;     /* >= 28*ceil(nEmig/1024)+28 */
	int *scratch;       /* >= 92 ints: [0] holes, [32, 60) base and [64, 92) count of each direction */
	double *buf;        /* 6*cap doubles */
	unsigned char *bufNe;
	long cap;
} pinc_extract_ws_t;
#define PINC_ERR_CAPACITY 77  /* *nEmig emigrants exceed ws.cap: grow and retry */
/* flag of a particle collected by an object in the fused push: extracted
 * like an emigrant, after every direction (neCount[PINC_NE_SINK]); neCount
 * has PINC_NE_CODES entries */
#define PINC_NE_SINK 27
#define PINC_NE_CODES 28
/* The flags of the extracted particles are set back to the centre, so that a
 * species' flags are all the centre again after its extraction. */
int pinc_hip_extract(pinc_pop_t pop, int s, unsigned char *flags, int *chunkCount,
                     int center, int nNeighbors, pinc_extract_ws_t ws, long *nEmig,
                     long *neCount, void *stream);

/* immersed objects (k_objects.hip; object.c, config C5).  inside: one byte
 * per node of the padded reference layout (strides 1, sy, sz; nNodes
 * nodes), the object id of interior nodes (0: none).  obj_flag writes
 * flags/chunk counts in pinc_hip_extract's format (flag 0 = remove, 13 =
 * keep) for oCollectObjectCharge (object.c:460-515) and adds the flagged
 * particles per object to objCount[id-1].  idx: device indices of the
 * surface nodes in a grid's slab storage.  obj_correct adds
 * sum_j M[j*n+i] (phiC - phiS[j]) to rho[idx[i]] (object.c:349-362). */
int pinc_hip_obj_flag(pinc_pop_t pop, int s, const unsigned char *inside, long sy, long sz, long nNodes,
                      unsigned char *flags, int *chunkCount, int *objCount, void *stream);
int pinc_hip_obj_gather(const double *grid, const long *idx, long n, double *out, void *stream);
int pinc_hip_obj_correct(const double *M, const double *phiS, long n, double phiC, const long *idx, double *rho,
                         void *stream);
int pinc_hip_obj_add(double *grid, const long *idx, long n, double v, void *stream);

/* multi-rank migration payload: records of 7 doubles (nd positions, nd
 * velocities, padding, direction) packed from buffer entries [first,
 * first+n), and appended to species s at index dst with the receiver's
 * shift (1-digit_d(ne))*T_d in every dimension (pusher.c:941-985) */
#define PINC_REC 7
int pinc_hip_pack(const double *buf, long cap, const unsigned char *bufNe, long first, long n,
                  int nd, double *out, void *stream);
int pinc_hip_import_rec(pinc_pop_t pop, int s, long dst, const double *rec, long n,
                        const int *shiftT, void *stream);

/* importParticles + shiftImmigrants (pusher.c:941-985): append n buffered
 * particles (buffer entries [first, first+n)) at index dst of species s,
 * shifting each position by -(digit_d(ne)-1)*T_d for the dims that wrap
 * locally (shiftMask bit d set). */
int pinc_hip_import(pinc_pop_t pop, int s, long dst, const double *buf, long cap,
                    const unsigned char *bufNe, long first, long n,
                    const int *shiftT, int shiftMask, void *stream);

/* CIC charge assignment puDistr3D1 / puDistrND1 (pusher.c:512-638) into the
 * slab grid; accumulates raw weights of species s (the caller applies the
 * reference's 1/q, q rescaling with pinc_hip_scale). */
int pinc_hip_deposit(pinc_pop_t pop, int s, pinc_geom_t g, double *rhoSlab, void *stream);

/* The first velocity moments of species s on the grid (an extension, not in
 * the reference), with the CIC weights w_j(x_p) of puDistr3D1 / puDistrND1
 * (particle p, node j).  Per node NM(nd) = 1 + nd + nd (nd + 1) / 2 doubles
 * (10, 6, 3), value-major as E holds its three:
 *   M[0]           = sum_p w_j(x_p)                  number per node
 *   M[1 + i]       = sum_p w_j(x_p) v_p,i            i < nd
 *   M[1 + nd + k]  = sum_p w_j(x_p) v_p,i v_p,j      i <= j, row-major upper
 *                    triangle: xx xy xz yy yz zz (3-D), xx xy yy (2-D), xx
 * Raw sums in code units (cells, cells per step), no charge or mass factor;
 * g.literal is ignored.  Positions are pop.x; v[d] are the velocity arrays
 * to read, indexed like pop.v[d] (pop.v itself in the plain case; element 0
 * 16-byte aligned, as pop.v[d]).  Accumulates into momSlab (a slab grid of NM
 * values per node, not zeroed here); the slab's ghost planes are left to the
 * caller's fold (pinc_hip_fold_self_values).  Precondition as
 * pinc_hip_deposit: every live particle's cell is in 0..T_d per dimension (a
 * cell outside is clamped to that range). */
int pinc_hip_moments(pinc_pop_t pop, int s, pinc_geom_t g, const double *const v[3], double *momSlab, void *stream);

/* Phase-space histogram of species s over one or two of its coordinates (an
 * extension, not in the reference).  The binning rule is fixed, so that it
 * can be restated bit for bit (no fused multiply-add in this library): per
 * axis a, with c the particle's coordinate,
 *     t = ((c + shift[a]) - lo[a]) * scale[a]            in fp64, this order
 * the particle is inside iff t >= 0 && t < nbins[a] on every axis (a NaN is
 * outside), its bin is (int)t, and it adds 1 to hist[b1 * nbins[0] + b0];
 * every other live particle adds 1 to *outside.  hist and outside are device
 * memory and are accumulated, not cleared.  Only [iStart[s], iStop[s]) is
 * read.  v[d] are the velocity arrays, as in pinc_hip_moments.  Errors: an
 * axis that is no PINC_PS_*, a position or velocity axis >= pop.nd,
 * nbins < 1, nbins[1] != 1 without a second axis, nbins[0] * nbins[1] > 2^24. */
enum { PINC_PS_X = 0, PINC_PS_Y, PINC_PS_Z, PINC_PS_VX, PINC_PS_VY, PINC_PS_VZ, PINC_PS_NONE = -1 };
typedef struct {
	int axis[2];     /* PINC_PS_*; axis[1] = PINC_PS_NONE for a 1-D histogram */
	int nbins[2];    /* nbins[1] = 1 when axis[1] is NONE */
	double shift[2]; /* added to the coordinate first (global-frame offset for a position, 0 for a velocity) */
	double lo[2];    /* lower edge */
	double scale[2]; /* nbins / (hi - lo), computed once by the caller */
} pinc_phase_t;
int pinc_hip_phase_hist(pinc_pop_t pop, int s, const double *const v[3], pinc_phase_t spec, unsigned long long *hist,
                        unsigned long long *outside, void *stream);
/* counters of the kernel's LDS box: a chunk of particles whose bounding box
 * in bin space has at most this area is counted in LDS (tests, the probe) */
long pinc_hip_phase_lds_bins(void);

/* E as the reference holds it while species s is accelerated: its sequence
 * of in-place gMul(E, q/m) ... gMul(E, m/q) (pusher.c:192,212) gives
 * Es = E*pre; for t<s: Es = (Es*qm[t])*mq[t]; Es *= qm[s] (same rounding).
 * n doubles of the slab E grid; qm/mq are device arrays. */
int pinc_hip_field_chain(const double *E, double *Es, long n, const double *qm, const double *mq,
                         double pre, int s, void *stream);
/* Every species' Es of pinc_hip_field_chain in one pass over E (the same
 * running chain, bit-identical): species s at Es + s n, s < nSpecies. */
int pinc_hip_field_chain_all(const double *E, double *Es, long n, const double *qm, const double *mq, double pre,
                             int nSpecies, void *stream);

/* order 0 (nearest grid point, node (int)(x + 0.5)): puDistrND0
 * (pusher.c:640-668) adds one unit per particle of species s (the caller
 * applies the 1/q, q chain); puAccND0KE (pusher.c:310-353, puInterpND0
 * :1164-1180) v += Es at the node, KE partials as pinc_hip_accelerate */
int pinc_hip_deposit_ngp(pinc_pop_t pop, int s, pinc_geom_t g, double *rhoSlab, void *stream);
int pinc_hip_accelerate_ngp(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, double *kePartial,
                            int *nBlocks, void *stream);
/* order 2 (quadratic B-spline, "TSC": three nodes per dimension), an
 * extension: the reference's puSanity (pusher.c:1047-1087) anticipates the
 * order without shipping its operators.  The weighting rule is fixed, so that
 * it can be restated exactly (no fused multiply-add in this library).  Per
 * dimension d, with T_d the true nodes (nloc in the slab dimension) and x_d
 * the position in the local frame, in fp64 and this order:
 *     j    = min(max((int)(x_d + 0.5), 1), T_d)      nearest true node, clamped
 *     dl   = x_d - j
 *     w[0] = 0.5 * ((0.5 - dl) * (0.5 - dl))         node j - 1
 *     w[1] = 0.75 - dl * dl                          node j
 *     w[2] = 0.5 * ((0.5 + dl) * (0.5 + dl))         node j + 1
 * A node's weight is the product of its per-dimension weights taken in the
 * order d = nd-1 .. 0: w_0 * (w_1 * w_2) in 3-D, w_0 * w_1 in 2-D.  That gives
 * 3^nd nodes in padded coordinates 0 .. T_d + 1, for positions in
 * [0.5, T_d + 0.5) (grid:thresholds = 0.5 with the one ghost layer).  The
 * clamp is part of the rule: at dl = +-0.5 the weights relative to j equal
 * those relative to j +- 1, so the rule is continuous at the clamp, and a
 * position that rounding has put on T_d + 0.5 still lands on nodes <= T_d + 1.
 *   deposit_tsc     adds the raw weights of species s to rhoSlab (accumulated,
 *                   never cleared; the caller applies the 1/q, q chain);
 *                   g.literal multiplies each node's weight as
 *                   pinc_hip_deposit_ngp does
 *   accelerate_tsc  dv_d = sum over the nodes of w Es[node nd + d], the nodes
 *                   in the order i_0 + 3 i_1 + 9 i_2 ascending; v += dv, KE
 *                   partials of v.(v + dv) as pinc_hip_accelerate_ngp (at most
 *                   ceil(n / 2048) blocks)
 * Errors (nothing is launched): nd outside 1..3, s outside the population's
 * species, a null array. */
int pinc_hip_deposit_tsc(pinc_pop_t pop, int s, pinc_geom_t g, double *rhoSlab, void *stream);
int pinc_hip_accelerate_tsc(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es, double *kePartial,
                            int *nBlocks, void *stream);
/* Monte Carlo collisions of species s with a uniform neutral background (an
 * extension: the reference has no collision module).  Null-free and direct:
 * every live particle is tested in every launch, against a neutral drawn for
 * it.  Process 0 is elastic (isotropic in the centre-of-mass frame), process 1
 * charge exchange (the particle takes the neutral's velocity).  Ionisation,
 * which creates particles, is pinc_hip_ionize's, below.  The rule is fixed, so
 * that it can be restated (tests/collide_ref.py):
 *   parameters   nu[k]    constant rate of process k per step
 *                sig[k]   n_n sigma_k per unit of path
 *                b = m_n / (m_s + m_n), a = 1 - b
 *                vth, drift[d]   the neutrals' Maxwellian
 *                h[d] = stepSize[d] / stepSize[0]
 *   Code velocities v_d are cells of dimension d per step; the physics is done
 *   on w_d = h_d v_d, and vth, drift and sig are in units of stepSize[0] and
 *   the time step.
 *   draws        key = pinc_hip_collide_key(seed, step, rank, s)
 *                    = mix64(mix64(seed ^ mix64(step)) ^ mix64(rank PINC_MAX_SPECIES + s))
 *                u_k = uni(key, 8 j + k), k = 0..7, for the particle at the
 *                species-local index j = i - iStart[s] (mix64 and uni: the
 *                counter RNG of pinc_hip_init_species).  Counter-based: a draw
 *                that is not needed is not made, with the same result.
 *   per particle, nd velocity components, in fp64:
 *     1. R = sqrt(-2 ln u4), N_0 = R cos(2 pi u5), N_1 = R sin(2 pi u5),
 *        N_2 = sqrt(-2 ln u6) cos(2 pi u7); n_d = drift_d + vth N_d, d < nd
 *     2. g_d = w_d - n_d, g = sqrt(sum g_d^2)
 *     3. r_k = nu_k + sig_k g, r = r_0 + r_1, P = -expm1(-r); the particle
 *        collides iff u0 < P
 *     4. elastic iff u1 r < r_0, else charge exchange
 *     5. charge exchange: w' = n.  Elastic: w'_d = a w_d + b n_d + b g e_d
 *        with the unit vector e
 *          nd = 3: c = 1 - 2 u2, s = sqrt((1 - c)(1 + c)), phi = 2 pi u3,
 *                  e = (s cos phi, s sin phi, c)
 *          nd = 2: phi = 2 pi u2, e = (cos phi, sin phi)
 *          nd = 1: e = +1 if u2 < 0.5, else -1
 *     6. v'_d = w'_d / h_d
 *   (cos and sin of 2 pi u are evaluated as cospi(2 u), sinpi(2 u); products
 *   and sums are not fused.)
 * A particle that does not collide is not written; positions are never read
 * or written.  v[d] are the velocity arrays, as in pinc_hip_moments (indexed
 * like pop.v[d], element 0 16-byte aligned).  counts[k] += the particles that
 * underwent process k in this launch (device memory, accumulated, not
 * cleared).  Errors (nothing is launched): s outside the population's species,
 * nd outside 1..3, a null array or counter, a negative or non-finite rate or
 * vth, a non-finite drift, b outside [0, 1], h_d <= 0. */
typedef struct {
	double nu[2];
	double sig[2];
	double b;
	double vth;
	double drift[3];
	double h[3];
	unsigned long long key;
} pinc_collide_t;
int pinc_hip_collide(pinc_pop_t pop, int s, double *const v[3], pinc_collide_t params, unsigned long long *counts,
                     void *stream);
/* the key of a launch (a pure host function: no device, no state) */
unsigned long long pinc_hip_collide_key(unsigned long long seed, unsigned long long step, int rank, int s);
/* particles per workgroup of pinc_hip_collide (a build constant; tests) */
long pinc_hip_collide_chunk(void);
/* Electron-impact ionisation of the same neutral background by species s (an
 * extension): a projectile faster than a threshold, relative to a neutral
 * drawn for it, loses the threshold energy, and an electron of species s and
 * an ion of species `target` are born where it stands.  The neutral is taken
 * as infinitely heavy, and what is left of the relative energy is shared by
 * the two electrons.  Every live particle is tested in every launch.  The rule
 * is fixed, so that it can be restated (tests/ionize_ref.py):
 *   parameters   nu       constant ionisation rate per step
 *                sig      n_n sigma per unit of path
 *                wth      threshold speed
 *                vth, drift[d], h[d]   as pinc_collide_t
 *                target   the species that receives the ions, != s
 *   Units as at pinc_hip_collide: the physics is done on w_d = h_d v_d; wth,
 *   vth, drift and sig are in units of stepSize[0] and the time step.
 *   draws        key = pinc_hip_ionize_key(seed, step, rank, s)
 *                    = mix64(pinc_hip_collide_key(seed, step, rank, s) ^ 0x696F6E697365)
 *                u_k = uni(key, 16 j + k), k = 0..15, for the particle at the
 *                species-local index j = i - iStart[s] (mix64, uni: as
 *                pinc_hip_collide).  Counter-based: a draw that is not needed
 *                is not made, with the same result.
 *   per live particle, nd components, in fp64, for d ascending:
 *     1. the neutral n_d exactly as in step 1 of pinc_hip_collide, from u4..u7
 *        of this stream
 *     2. w_d = h_d v_d, g_d = w_d - n_d, G = sum g_d^2, g = sqrt(G)
 *     3. r = nu + sig g, P = -expm1(-r), W = wth wth; the particle ionises
 *        iff G > W && u0 < P
 *     4. rem = G - W, f = u1, g1 = sqrt(f rem), g2 = sqrt((1 - f) rem)
 *     5. unit vectors by step 5 of pinc_hip_collide for this nd: e1 from
 *        (u2, u3), e2 from (u8, u9)
 *     6. the parent gets v'_d = (n_d + g1 e1_d) / h_d; the new electron
 *        (n_d + g2 e2_d) / h_d and the new ion n_d / h_d, both at the parent's
 *        position, copied bit for bit.  In the neutral's frame
 *        |w' - n|^2 + |w_new - n|^2 = G - W.
 *   (cospi, sinpi as at pinc_hip_collide; products and sums are not fused.)
 * Placement: the births of a launch are numbered k = 0, 1, ... in ascending
 * parent index; birth k writes the electron to slot iStop[s] + k and the ion to
 * slot iStop[target] + k.  Only [iStart[s], iStop[s]) as passed in is tested.
 * The ranges are the host's: the kernel does not change them, and the caller
 * adds the births (res[0]'s increase) to both iStop.  res is device memory:
 * res[0] += the births of this launch.  If they exceed the free slots of either
 * species (iStart[q + 1] - iStop[q]), nothing is written: no parent, no child,
 * not res[0]; res[1] is set to 1 and the call still returns 0.  A particle that
 * does not ionise is not written; positions of existing particles are never
 * written.  work: pinc_hip_ionize_work(n) ints of device scratch for n live
 * particles (workInts of them are there).  Errors (nothing is launched): s or
 * target outside the population's species, or equal; nd outside 1..3; a null
 * array; a live range outside its species' slots; work too small; a negative
 * or non-finite nu, sig, wth or vth; a non-finite drift; h_d <= 0. */
typedef struct {
	double nu;        /* constant ionisation rate per step */
	double sig;       /* n_n sigma per unit of path */
	double wth;       /* threshold speed, in stepSize[0] per step */
	double vth, drift[3], h[3];   /* as pinc_collide_t */
	int target;       /* species that receives the ions, != s */
	unsigned long long key;
} pinc_ionize_t;
int pinc_hip_ionize(pinc_pop_t pop, int s, pinc_ionize_t par, int *work, long workInts, unsigned long long *res,
                    void *stream);
/* ints of scratch for n live particles */
long pinc_hip_ionize_work(long n);
/* particles per workgroup of pinc_hip_ionize (a build constant; tests) */
long pinc_hip_ionize_chunk(void);
/* the key of a launch (a pure host function: no device, no state) */
unsigned long long pinc_hip_ionize_key(unsigned long long seed, unsigned long long step, int rank, int s);
/* Binary Coulomb collisions between the particles of species a and b, a <= b
 * (Takizuka & Abe 1977; an extension).  One launch treats one ordered pair of
 * species; a == b is like-particle scattering.  The particles of a cell are
 * paired with each other, and every pair scatters by an angle drawn for it.
 * 3-D only (the scattering needs three velocity components).  The rule is
 * fixed, so that it can be restated (tests/coulomb_ref.py):
 *   parameters   K        the pair's coefficient K_ab;
 *                         K == 0 switches the pair off: nothing is launched
 *                fa, fb   the mass fractions mu / m_a and mu / m_b of the
 *                         reduced mass mu (fa + fb = 1 for the host's values;
 *                         1/2 each for a like pair)
 *                h[d] = stepSize[d] / stepSize[0]
 *   Units as at pinc_hip_collide: the physics is done on w_d = h_d v_d, results
 *   go back as v_d = w_d / h_d; fp64 throughout, products and sums are not
 *   fused, cos and sin of pi t are cospi(t) and sinpi(t).
 *   cell         with T_d the rank's true cells (g.T[d], g.nloc for d = 2),
 *                c_d = min(max((int)x_d, 1), T_d) - 1 and
 *                cell = c_0 + T_0 (c_1 + T_1 c_2): the integer cell of the
 *                position in the local frame, clamped to the true cells.  It
 *                differs from the cell pinc_hip_count_keys counts in two
 *                ways: that one is the cell of x + v (where the next push
 *                takes the particle) and is clamped to the ghost layer 0..T+1.
 *                Positions are read, never written.
 *   keys         key = pinc_hip_coulomb_key(seed, step, rank, a, b)
 *                    = mix64(pinc_hip_collide_key(seed, step, rank, a)
 *                            ^ 0x636F756C6F6D62 ^ mix64(a PINC_MAX_SPECIES + b))
 *                key_s    = mix64(key ^ 1) for species a, mix64(key ^ 2) for b
 *                key_pair = mix64(key ^ 3) where the first-named particle of a
 *                           collision is of species a, mix64(key ^ 4) where it
 *                           is of species b (a != b)
 *                (mix64, uni: the counter RNG of pinc_hip_collide.)
 *   order        the members of species s in a cell, sorted ascending by
 *                (mix64(key_s ^ mix64(j)), j), j the species-local index
 *                i - iStart[s]: a total order that does not depend on how the
 *                members were gathered.
 *   like pairs (a == b), the cell's list L of length N:
 *                N < 2: nothing.  N even: the pairs (L[2m], L[2m+1]).  N odd:
 *                the triple (L0, L1), (L1, L2), (L2, L0), applied in that
 *                order, each with f = 1/2 and on the velocities the one before
 *                left; then (L[3+2m], L[4+2m]).
 *   unlike pairs (a < b): A is the longer list and B the shorter, A that of
 *                species a on equal lengths.  With Q = |A| / |B| (integer) and
 *                R = |A| mod |B|, B[k] collides in turn with Q + 1 consecutive
 *                members of A for k < R and with Q otherwise, walking A in
 *                order from A[0]; it carries its velocity from one partner to
 *                the next.  An empty B: nothing.
 *   one collision of p (first-named: L[2m]; L0, L1, L2 for the triple's three
 *   pairs; the A-member) with q, f = 1 outside a triple:
 *     1. g_d = w_p,d - w_q,d; gp = sqrt(gx gx + gy gy),
 *        g = sqrt((gx gx + gy gy) + gz gz).  No collision if g == 0.
 *     2. var = ((K nLow) f) / ((g g) g), nLow the shorter of the two lists'
 *        lengths in this cell (N for a like pair)
 *     3. u_k = uni(key_pair, 4 j + k), j the species-local index of p: every
 *        collision of a launch has a counter block of its own (u3 is not used)
 *     4. var < 1:  dl = (sqrt(var) sqrt(-2 ln u0)) cospi(2 u1),
 *                  sinT = 2 dl / (1 + dl dl), omc = 2 dl dl / (1 + dl dl)
 *        else:     c = 1 - 2 u0, sinT = sqrt((1 - c)(1 + c)), omc = 1 - c
 *        (omc = 1 - cos Theta), cphi = cospi(2 u2), sphi = sinpi(2 u2)
 *     5. gp > 0:   Dx = (gx/gp) gz sinT cphi - (gy/gp) g sinT sphi - gx omc
 *                  Dy = (gy/gp) gz sinT cphi + (gx/gp) g sinT sphi - gy omc
 *                  Dz = -gp sinT cphi - gz omc
 *        gp == 0:  D = (gz sinT cphi, gz sinT sphi, -gz omc)   (g = |gz|; the
 *                  sign of gz is kept, so that |g + D| = g in both directions)
 *     6. w_p += (mu / m_p) D, w_q -= (mu / m_q) D
 * counts[0] += the collisions applied in this launch (device memory,
 * accumulated, not cleared); a pair with g == 0 is not counted and not
 * written.  Only velocities of particles that collided are written.  work:
 * pinc_hip_coulomb_work(nA, nB, nCells) ints of device scratch for the live
 * particles of the two species (nB = 0 for a == b) and the rank's true cells.
 * Errors (nothing is launched): a or b outside the population's species, or
 * a > b; nd != 3 (population or geometry); a null array, scratch or counter;
 * work too small; a negative or non-finite K; a mass fraction outside (0, 1);
 * h_d <= 0. */
typedef struct {
	double K;
	double fa, fb;    /* mu / m_a, mu / m_b */
	double h[3];      /* as pinc_collide_t */
	unsigned long long key;
} pinc_coulomb_t;
int pinc_hip_coulomb(pinc_pop_t pop, int a, int b, pinc_geom_t geom, pinc_coulomb_t params, int *work, long workInts,
                     unsigned long long *counts, void *stream);
/* ints of scratch */
long pinc_hip_coulomb_work(long nA, long nB, long nCells);
/* the longest cell list a wave orders in LDS (a build constant; tests): a
 * longer one is ordered from global memory, with the same result */
long pinc_hip_coulomb_cell_cap(void);
/* the key of a launch (a pure host function: no device, no state) */
unsigned long long pinc_hip_coulomb_key(unsigned long long seed, unsigned long long step, int rank, int a, int b);
/* pVelAssertMax (population.c:342-365) over species s: a velocity component
 * above maxVel sets bit 0 of *errFlag */
int pinc_hip_vel_assert(pinc_pop_t pop, int s, double maxVel, int *errFlag, void *stream);
/* particles per workgroup of pinc_hip_push (a build constant) */
long pinc_hip_push_chunk(void);
/* xcd[c] = the XCD (block index mod 8) whose block processes push chunk c,
 * for a launch of nBlocks blocks (the push's chunk placement; trace
 * diagnostics) */
int pinc_hip_push_xcd_of_chunks(long nBlocks, int *xcd);

/* puAcc3D1KE / puAccND1KE (pusher.c:178-265) with puInterp3D1/ND1
 * (pusher.c:1089-1162), gathering from Es (pinc_hip_field_chain).
 * kePartial receives per-block partial sums of v.(v+dv) (at most
 * ceil((n+1)/2048) blocks); nBlocks returned. */
int pinc_hip_accelerate(pinc_pop_t pop, int s, pinc_geom_t g, const double *Es,
                        double *kePartial, int *nBlocks, void *stream);

/* device-side initial conditions (pPosLattice population.c:172-240,
 * pPosPerturb 242-276, pVelZero/Maxwell): generates the lattice indices of
 * this rank, optional cosine perturbation, zero or Maxwellian velocities
 * from the counter RNG shared with the oracle.  Returns count in *n. */
int pinc_hip_init_species(pinc_pop_t pop, int s, pinc_geom_t g, long nGlobal, double latticeStep,
                          const int *subdomain, const int *nSubdomains, const int *offset,
                          const double *amp, const double *mode, int perturb,
                          int maxwell, double drift, double vth, unsigned long long seed,
                          long *n, void *stream);

/* -------------------------------------------------------------- grids -- */
int pinc_hip_zero(double *a, long n, void *stream);
int pinc_hip_scale(double *a, long n, double f, void *stream);
/* a = (a*f1)*f2 in one pass (two roundings, as two gMul calls) */
int pinc_hip_scale2(double *a, long n, double f1, double f2, void *stream);
/* gHaloOp(addSlice, rho, FROMHALO) along the slab dim for a self-periodic
 * slab (grid.c:340-406): plane 0 += into nloc, plane nloc+1 += into 1 */
int pinc_hip_fold_self(double *slab, pinc_geom_t g, void *stream);
/* the same for a value-major slab of nValues doubles per node */
int pinc_hip_fold_self_values(double *slab, pinc_geom_t g, int nValues, void *stream);
/* a += b elementwise (gAddTo, grid.c:781-789) */
int pinc_hip_add(double *a, const double *b, long n, void *stream);
/* every slab node (incl. ghost planes) from the global periodic grid:
 * gHaloOp(setSlice, TOHALO) for a grid whose truth lives in the global
 * array (phi after the solve) */
int pinc_hip_slab_from_global(double *slab, const double *global, pinc_geom_t g, int nValues,
                              void *stream);
/* add a received plane into a slab plane */
int pinc_hip_add_plane(double *slab, pinc_geom_t g, int plane, const double *in, void *stream);
int pinc_hip_copy_plane(double *dst, const double *slab, pinc_geom_t g, int plane, int nValues, void *stream);
/* gFinDiff1st + TOHALO (grid.c:226-261, main.c:245-246):
 * E = 0.5*(phi[+d]-phi[-d]) on every slab plane incl. ghosts, from the
 * global periodic phi (ghost planes then equal the neighbours' values
 * bit for bit, so the TOHALO is implied). */
int pinc_hip_efield(const double *phiGlobal, pinc_geom_t g, double *Eslab, void *stream);
/* The same with E = h (phi_up - phi_dn): h = 0.5 is pinc_hip_efield, h = -0.5
 * its result followed by gMul(E, -1) (main.c:247) bit for bit, in one pass
 * (regular()'s step); other h are rejected. */
int pinc_hip_efield_scaled(const double *phi, pinc_geom_t g, double *E, double h, void *stream);
/* deterministic two-stage sums: *out = sum(a) ; sum(a*b) */
int pinc_hip_sum(const double *a, long n, double *partial, double *out, void *stream);
int pinc_hip_dot(const double *a, const double *b, long n, double *partial, double *out, void *stream);
/* *out = sum(a)/div  (the mean of gNeutralizeGrid, grid.c:746) */
int pinc_hip_sum_div(const double *a, long n, double div, double *partial, double *out, void *stream);
/* *out = (sum of the first n entries of partial) / div */
int pinc_hip_reduce(const double *partial, int n, double div, double *out, void *stream);

/* --------------------------------------------------------- multigrid -- */
/* One level of the global periodic grid. */
typedef struct { int nd; int T[3]; } pinc_lvl_t;
/* Red-black Gauss-Seidel colour pass (mgGS3D multigrid.c:683-767 when nd3,
 * mgGSND 553-621 otherwise) on true points of colour `pass`, reading the
 * other colour with the pending neutralisation shift *muPrev (exactly the
 * reference's stored value - mu), writing block partial sums of the
 * resulting logical grid into partial. nBlocks returned. */
int pinc_hip_gs_pass(double *phi, const double *rho, pinc_lvl_t L, int pass, int nd3,
                     const double *muPrev, double *partial, int *nBlocks, void *stream);
/* phi = (phi - muA) - muB on colour `pass`'s complement and phi - muB on
 * colour `pass` (materialise pending shifts after a smoothing sequence) */
/* Native mode (multigrid:native): one full red-black iteration of mgGS3D
 * without the per-colour neutralisation, phiIn -> phiOut (distinct buffers),
 * in one pass; bit-identical to two pinc_hip_gs_pass calls with muPrev NULL.
 * Needs a 3-D level with T[0], T[1], T[2] multiples of 16. */
int pinc_hip_gs_sweep(const double *phiIn, double *phiOut, const double *rho, pinc_lvl_t L,
                      void *stream);
/* Native mode: two full red-black iterations phiIn -> phiOut in one pass
 * (z-march four stages deep); bit-identical to two pinc_hip_gs_sweep calls.
 * Needs T[0] % 32, T[1] % 8 and T[2] % 16 == 0. */
int pinc_hip_gs_sweep2x(const double *phiIn, double *phiOut, const double *rho, pinc_lvl_t L,
                        void *stream);
/* Native mode: the whole V-cycle below (and including) a coarse level in one
 * 1024-thread workgroup, grids in LDS (at most 5500 points over all levels,
 * 1-D to 3-D, each level half the previous in every dimension).  levels[0]
 * is the top coarse level: its rho is read from `rho`, its correction starts
 * at zero and is written to `phi`; rho of the levels below is the restricted
 * residual times 4.  hw3d / gs3d select mgHalfRestrict3D / mgGS3D's forms
 * (3-D only), else the ND forms. */
/* Native mode, one rank, a 2-D level 0 of T0 x T1 <= 16384 points (T0 a
 * power of two, T1 even, T0 T1 a multiple of 2048; mgGSND form, the ND
 * restriction), levels 1.. within k_mg_coarse's LDS budget: whole V-cycles
 * of levels[0..nLevels) from phi (initial guess, in/out) with rho, in one
 * workgroup, until the RMS residual is <= tol or maxCycles ran; res (T0 T1
 * doubles) is scratch.  out[0] = cycles, out[1] = the last RMS residual,
 * out[2 + c] = the residual after cycle c (c < 60).  coarseBasis NULL: the
 * V-cycle of the per-level launches (k_mg_coarse for levels 1..);
 * otherwise the two-grid cycle of multigrid:spectralCoarse with level 1
 * (square, n = 16..64 in 16s) solved exactly: coarseBasis holds the real
 * orthonormal Fourier basis Q (n x n, row-major, Q[j][k]) and then the n
 * eigenvalues 2 - 2 cos(2 pi f_k / n) of its columns. */
int pinc_hip_mg_solve_small(double *phi, const double *rho, double *res, int nLevels, const pinc_lvl_t *levels,
                            int nPre, int nPost, int nCoarse, int maxCycles, double tol, const double *coarseBasis,
                            double *out, void *stream);
int pinc_hip_mg_coarse(const double *rho, double *phi, int nLevels, const pinc_lvl_t *levels, int nPre,
                       int nPost, int nCoarse, int hw3d, int gs3d, void *stream);
/* Sharded level 0 of the native multigrid (several ranks, 3-D): this rank's
 * z-slab extended by halo planes, Lx = T0 x T1 x (nloc + 2 hz), x/y periodic,
 * z neighbours read directly.
 *   residual_slab        residual on planes [zlo, zhi) of the extended slab
 *   residual_sumsq_slab  block partials of its square (RMS norm)
 *   restrict_slab        this rank's level-1 planes (Lc: T0/2 x T1/2 x nloc/2)
 *                        from the slab's residual starting at plane zf0,
 *                        times 4 (coarse h^2 factor)
 *   prolong_add_slab     every slab plane += the global level-1 correction
 *                        (Lc global); slab plane zl is global plane z0 + zl
 *                        (mod Tz)
 *   prolong_add_own      the owned planes [hz, hz + nloc) += the correction
 *                        of this rank's own level-1 planes, held in phiCx
 *                        with one halo plane on each side (Lcx: T0/2 x T1/2
 *                        x (nloc/2 + 2)); level 1 decomposed as level 0 */
int pinc_hip_residual_slab(double *res, const double *phi, const double *rho, pinc_lvl_t Lx, int zlo, int zhi,
                           void *stream);
int pinc_hip_residual_sumsq_slab(const double *phi, const double *rho, pinc_lvl_t Lx, int zlo, int zhi,
                                 double *partial, int *nBlocks, void *stream);
int pinc_hip_restrict_slab(const double *fineX, pinc_lvl_t Lx, int zf0, double *coarse, pinc_lvl_t Lc, int nd3,
                           void *stream);
int pinc_hip_prolong_add_slab(double *phiX, pinc_lvl_t Lx, int z0, int Tz, const double *phiC, pinc_lvl_t Lc,
                              void *stream);
int pinc_hip_prolong_add_own(double *phiX, pinc_lvl_t Lx, int hz, int nloc, const double *phiCx, pinc_lvl_t Lcx,
                             void *stream);
int pinc_hip_gs_materialize(double *phi, pinc_lvl_t L, int lastPass, const double *muA,
                            const double *muB, void *stream);
/* phi -= *mu over all points */
int pinc_hip_sub_dev(double *a, long n, const double *mu, void *stream);
/* multigrid:extrapolate (native mode, an extension): phi <- 2 phi - prev and
 * prev <- old phi over n values, the initial guess of the next solve from the
 * last two solutions (mgSolveRaw, multigrid.c:1688-1724, warm-starts from the
 * last one) */
int pinc_hip_extrapolate(double *phi, double *prev, long n, void *stream);
/* out = a x + b y over n values (out may alias x or y) */
int pinc_hip_lincomb(double *out, const double *x, double a, const double *y, double b, long n, void *stream);
/* mgResidual (multigrid.c:1385-1403): res = lap(phi) + rho */
int pinc_hip_residual(double *res, const double *phi, const double *rho, pinc_lvl_t L,
                      void *stream);
/* residual sum of squares only (mgSumTrueSquared, multigrid.c:1471-1481) */
int pinc_hip_residual_sumsq(const double *phi, const double *rho, pinc_lvl_t L,
                            double *partial, int *nBlocks, void *stream);
/* mgHalfRestrict3D / ND (multigrid.c:844-1022) */
int pinc_hip_restrict(const double *fine, double *coarse, pinc_lvl_t Lc, int nd3, void *stream);
/* mgBilinProl3D/ND + gAddTo (multigrid.c:1024-1238, 1535): phi_f += P(phi_c) */
int pinc_hip_prolong_add(double *phiFine, const double *phiCoarse, pinc_lvl_t Lf, void *stream);
/* 3-D forms of the level transfers, one thread per coarse cell (bit-identical
 * to the point kernels above): coarse = scale * restrict(residual(phi, rho))
 * (mgResidual + mgHalfRestrict3D / ND without writing the fine residual;
 * scale 4 in native mode); phi_f += P(phi_c) for the coarse level Lc (phi_f
 * 16-byte aligned) */
int pinc_hip_resid_restrict(const double *phi, const double *rho, double *coarse, pinc_lvl_t Lc, int hw3d,
                            double scale, void *stream);
int pinc_hip_prolong_add3(double *phiFine, const double *phiCoarse, pinc_lvl_t Lc, void *stream);

/* ---------------------------------------------------------- spectral -- */
/* Spectral Poisson solve on rocFFT, replacing sAlloc/sSolve/sFree
 * (spectral.c:14-52, 92-115).  T is the global true size (x fastest, x
 * even).  pinc_hip_fft_poisson reads the global rho [Tz][Ty][Tx] (left
 * unchanged) and writes the global phi: r2c, DC := 0, multiply by
 * (N/(2 pi n))^2/N in 1-D (spectral.c:29-37) or 1/|k|^2/N in 2-D/3-D, c2r. */
typedef struct pinc_fft_s pinc_fft_t;
int pinc_hip_fft_create(pinc_fft_t **plan, int nd, const int *T, void *stream);
int pinc_hip_fft_poisson(pinc_fft_t *plan, const double *rhoGlobal, double *phiGlobal, void *stream);
void pinc_hip_fft_destroy(pinc_fft_t *plan);
/* symbol of the plan's k-space factor: 0 the spectral solver's (above), 1
 * the multigrid's 7-point (5-, 3-point) discrete Laplacian,
 * 1/sum_d (2 - 2 cos(2 pi n_d/N_d))/N: the exact discrete solution the
 * multigrid converges to (objects:secondGuess = spectral) */
int pinc_hip_fft_set_symbol(pinc_fft_t *plan, int discrete);

/* Slab-distributed 3-D spectral solve (several ranks,
 * z-slabs of nloc planes, Ty divisible by the rank count): the same operator
 * as pinc_hip_fft_poisson without gathering rho.
 *   forward   rho slab (nloc planes, x fastest) -> batched 2-D r2c -> the
 *             send buffer S, blocks [q][zl][yl][kx] (block q: ky rows
 *             [q Ty/P, (q+1) Ty/P))
 *   (host)    block q of S to rank q into block r of B on rank q
 *   kspace    B = [z][yl][kx]: c2c along z, the k-space factor, inverse c2c
 *   (host)    block q of B (z rows of slab q) to rank q into block r of S
 *   backward  S -> unpack -> batched 2-D c2r -> phi slab (nloc planes)
 * buffers: S and B device pointers, bytes per block (P blocks each). */
typedef struct pinc_fft_slab_s pinc_fft_slab_t;
int pinc_hip_fft_slab_create(pinc_fft_slab_t **plan, const int *T, int nloc, int nranks, int rank, void *stream);
int pinc_hip_fft_slab_buffers(pinc_fft_slab_t *plan, void **S, void **B, long *blockBytes);
/* the slab plan's symbol, as pinc_hip_fft_set_symbol (1: the multigrid's
 * 7-point Laplacian; the sharded multigrid's spectral second guess) */
int pinc_hip_fft_slab_set_symbol(pinc_fft_slab_t *plan, int discrete);
int pinc_hip_fft_slab_forward(pinc_fft_slab_t *plan, const double *rhoSlab, void *stream);
int pinc_hip_fft_slab_kspace(pinc_fft_slab_t *plan, void *stream);
int pinc_hip_fft_slab_backward(pinc_fft_slab_t *plan, double *phiSlab, void *stream);
void pinc_hip_fft_slab_destroy(pinc_fft_slab_t *plan);

/* ------------------------------------------------------------ comm -- */
/* RCCL communicator over xGMI (one process per GPU).  id is the 128-byte
 * ncclUniqueId produced by pinc_hip_comm_unique_id on rank 0 and
 * distributed by the launcher. */
#define PINC_COMM_ID_BYTES 128
int pinc_hip_comm_unique_id(unsigned char *id);
int pinc_hip_comm_init(void **comm, const unsigned char *id, int nranks, int rank);
int pinc_hip_comm_destroy(void *comm);
/* label of the next RCCL call for the watchdog's message (pinc_hip_comm_init
 * starts a watchdog thread: a call that has not completed after
 * PINC_COMM_TIMEOUT seconds, default 300, aborts the communicator and ends
 * the process with status 3) */
int pinc_hip_comm_note(const char *what);
int pinc_hip_comm_sendrecv(void *comm, const void *sendbuf, long sendBytes, int peerSend,
                           void *recvbuf, long recvBytes, int peerRecv, void *stream);
/* grouped point-to-point exchange: op i sends sendBytes[i] to sendPeer[i]
 * and receives recvBytes[i] from recvPeer[i].  Transfers between one pair of
 * ranks match in op order, so with two slabs (up == down) pair each send
 * with the receive from the opposite direction. */
int pinc_hip_comm_exchange(void *comm, int nOps, const int *sendPeer, void *const *sendbuf,
                           const long *sendBytes, const int *recvPeer, void *const *recvbuf,
                           const long *recvBytes, void *stream);
int pinc_hip_comm_allgather(void *comm, const double *send, double *recv, long count, void *stream);
int pinc_hip_comm_allreduce_sum(void *comm, const double *send, double *recv, long count, void *stream);
/* test hook: occupy the stream for `seconds` (at most 30) of wall time with a
 * one-lane kernel that ends by itself (tests/test_gpu_rccl_watchdog.py holds
 * an RCCL call behind it) */
int pinc_hip_test_spin(double seconds, void *stream);

#ifdef __cplusplus
}
#endif
#endif
