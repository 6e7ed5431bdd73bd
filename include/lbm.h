/*
 * lbm.h — C ABI of liblbm_hip.so: the MI355X-native D2Q9-BGK timestep.
 *
 * This is the drop-in boundary for the reference's host<->device seam.  The reference
 * (ag14774/OpenCL-Lattice-Boltzmann) has no plugin API; its hot path sits behind the OpenCL
 * calls made by d2q9-bgk.c.  Each entry point below replaces the cited call site(s); a host
 * written against this header needs no OpenCL, no kernels.cl and no JIT.
 *
 * Conventions
 *   - plain C, plain pointers and sizes, no C++/torch types;
 *   - every function returns LBM_OK (0) or a non-zero LBM_ERR_* code; lbm_last_error() returns
 *     the message of the calling thread's most recent failure (the reference's checkError()
 *     prints such a message and exits, d2q9-bgk.c:858-866 — the host does the same);
 *   - the caller owns all host arrays (d2q9-bgk.c:519-526,597,720-727); the library owns all
 *     device memory (d2q9-bgk.c:687-710,729-733);
 *   - one host thread drives a context; calls are asynchronous on the context's HIP streams and
 *     ordered like the reference's single in-order queue (d2q9-bgk.c:612-616);
 *   - cells layout = the reference's SoA: float[9][ny][nx], speed k at k*nx*ny + y*nx + x
 *     (d2q9-bgk.c:73, kernels.cl:7), speeds numbered 0 rest, 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW,
 *     7 SW, 8 SE (d2q9-bgk.c:7-13); obstacles = int32[ny][nx], 0 fluid / non-zero blocked.
 */
#ifndef LBM_H
#define LBM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_OK 0
#define LBM_ERR_ARG 1    /* bad argument */
#define LBM_ERR_HIP 2    /* HIP runtime error (message has the hipError string) */
#define LBM_ERR_STATE 3  /* call not valid in the context's current state */
#define LBM_ERR_COMM 4   /* halo transport error (RCCL, peer mapping, a neighbour that never arrived) */

/* Run constants: the reference's t_param (d2q9-bgk.c:81-92), same fields. */
typedef struct lbm_params {
  int nx;               /* cells in x */
  int ny;               /* cells in y */
  int max_iters;        /* capacity of the av_vels record (steps that can be run) */
  int reynolds_dim;     /* dimension for the Reynolds number */
  float density;        /* density per link */
  float accel;          /* density redistribution */
  float omega;          /* relaxation parameter */
  float free_cells_inv; /* 1 / number of non-blocked cells (d2q9-bgk.c:591) */
} lbm_params;

typedef struct lbm_ctx lbm_ctx; /* opaque; replaces t_ocl (d2q9-bgk.c:97-119) */

/*
 * Create a context: select device(s), allocate the two cell grids, the obstacle mask and the
 * reduction buffers.  Replaces selectOpenCLDevice + clCreateContext/Queue/Program/Kernel/Buffer
 * (d2q9-bgk.c:600-710, 885-944) and the obstacle upload (d2q9-bgk.c:205-209).
 *   obstacles  borrowed for the duration of the call.
 *   ndev       number of row slabs; the grid is row-partitioned over dev_ids[0..ndev).  ndev <= 1
 *              with dev_ids == NULL uses the current HIP device.  A device may be listed more than
 *              once (several slabs on one GPU).  Every slab needs at least 4 rows.  Halo rows move by
 *              the PEER transport (a kernel stores them straight into the neighbour slab's halo rows,
 *              peer access between distinct devices) unless lbm_set_default("transport") asks for
 *              RCCL send/recv (distinct devices only) or device-to-device copies.
 */
int lbm_create(lbm_ctx **out, const lbm_params *params, const int32_t *obstacles, int ndev, const int *dev_ids);

/*
 * One-process-per-GPU form (torchrun / MPI style launch): this process owns slab `rank` of
 * `nranks` on HIP device `device`; halos are exchanged with ranks (rank±1) mod nranks by RCCL
 * send/recv and the velocity sums are combined by an RCCL all-reduce.  `comm_id` is the
 * lbm_comm_id_size()-byte blob produced by lbm_comm_get_id() on one rank and distributed by the
 * caller (e.g. torch.distributed broadcast).  params/obstacles describe the GLOBAL grid.
 * No counterpart in the reference (single device); mandated by the multi-GPU configs.
 * comm_id == NULL creates the rank without RCCL communicator: it must then be connected with
 * lbm_connect_peers before the first lbm_run, and lbm_download returns the velocity sums over THIS rank's
 * rows only (times free_cells_inv) — the caller adds the ranks' records.
 */
int lbm_create_rank(lbm_ctx **out, const lbm_params *params, const int32_t *obstacles,
                    int rank, int nranks, int device, const void *comm_id);
size_t lbm_comm_id_size(void);
int lbm_comm_get_id(void *comm_id_out);

/*
 * PEER halo transport between ranks (the low-latency alternative to RCCL send/recv for the halo rows; the
 * all-reduce stays with RCCL).  Each rank describes its two grids and its flag words in an
 * lbm_peer_info_size()-byte blob (HIP IPC handles + the raw pointers for neighbours inside the same process);
 * the caller distributes the blobs (e.g. torch.distributed all_gather) and hands every rank the blobs of its ring
 * neighbours (rank-1) mod nranks and (rank+1) mod nranks.  From then on a launch set's edge rows are stored
 * straight into the neighbours' halo rows by a push kernel (xGMI peer writes) which then raises a sequence
 * number in the neighbour's flag word; the consumer waits for it with a bounded spin (30 s; reported by lbm_sync
 * as LBM_ERR_COMM) or hipStreamWaitValue32 (option "halo_sync").  lbm_connect_peers is a collective decision:
 * every rank of the ring must call it (or none).  A context WITHOUT communicator runs on peer stores from then on; a
 * context that also has an RCCL communicator stays on RCCL send/recv until lbm_set_option("transport", 3) (or default
 * "transport" = 3 at creation) — peer stores between devices are the caller's explicit choice, to be made once they
 * have been checked against the RCCL ring on the machine at hand (bench.py: transport_check); "transport" 1 | 3
 * switches back and forth.  A blob is recognised as "my own process" by a per-process random nonce + boot id, not by
 * the pid.  A failed call leaves nothing mapped; a repeated call unmaps the previous neighbours first.
 */
size_t lbm_peer_info_size(void);
int lbm_peer_info(lbm_ctx *ctx, void *info_out);
int lbm_connect_peers(lbm_ctx *ctx, const void *south_info, const void *north_info);
/*
 * Unmap the ring neighbours' grids and flag words (waits for this context's queued work first).  ORDER OF TEAR-DOWN
 * between processes: every rank calls lbm_disconnect_peers, the caller synchronises the ranks (a barrier), and only then
 * does any rank call lbm_destroy — freeing device memory that another process still has mapped through HIP IPC is
 * undefined behaviour (as with CUDA IPC).  lbm_destroy alone is enough inside one process and for a rank whose
 * neighbours have already gone.  Afterwards the context is back on RCCL send/recv if it has a communicator, else
 * without transport until lbm_connect_peers is called again.
 */
int lbm_disconnect_peers(lbm_ctx *ctx);

/*
 * Process-wide defaults for contexts created afterwards (validated; replace the environment hooks of round 1):
 *   "force_halo"  0 | 1   a single slab also carries halo rows and exchanges them with itself (a ring of one): the
 *                         whole multi-GPU machinery of a rank on one GPU (tests, tools/scaling_projection.py)
 *   "halo_depth"  0 = by slab size (8 small slabs and slabs from 3M cells / 4 from 2M cells / 3 / 2 thin slabs), else 2..8
 *   "transport"   0 = auto, 1 = RCCL send/recv, 2 = device-to-device copies, 3 = peer stores
 *   "lanes_out"   0 = auto (60), else 4..62: output lanes per 64-lane strip of the window kernels
 */
int lbm_set_default(const char *key, long value);

/*
 * Host -> device copy of the initial state.  Replaces clEnqueueWriteBuffer(cells)
 * (d2q9-bgk.c:200-203).  cells == NULL initialises the uniform rest state on the device
 * (the values of d2q9-bgk.c:529-550) without any host transfer.  Resets the step counter.
 * In rank mode `cells` is the GLOBAL array; only this rank's rows are read.
 */
int lbm_upload(lbm_ctx *ctx, const float *cells);

/*
 * Host -> device copy of the obstacle map: replaces clEnqueueWriteBuffer(obstacles) (d2q9-bgk.c:205-209).  lbm_create
 * has already taken the map it was given (it needs it to lay out the slabs); this entry point exists so that a host
 * that follows the reference's timing rule — everything from the first host->device transfer to the last read-back
 * inside the timed region, d2q9-bgk.c:196-263 — can have the obstacle transfer inside it, and so that a caller may
 * change the map between runs (same nx, ny; params.free_cells_inv is the caller's to keep consistent: it was fixed
 * at lbm_create).  obstacles = int32[ny][nx] of the GLOBAL grid, borrowed.  Synchronises.  Also rebuilds what the library
 * derives from the map (the per-strip bits of rows with blocked cells that option "free_sweeps" consults: one kernel, ~75 us
 * at 8192 x 8192).
 */
int lbm_upload_obstacles(lbm_ctx *ctx, const int32_t *obstacles);

/*
 * Advance nsteps timesteps (accelerate_flow + timestep + av_vels reduction each); asynchronous.
 * Replaces the loop body d2q9-bgk.c:221-238 (accelerate_flow(), timestep(), reduce() wrappers,
 * d2q9-bgk.c:282-393).  May be called repeatedly; after n calls' worth of steps exactly that many
 * steps have been applied and av_vels[t] is defined for every one of them.
 */
int lbm_run(lbm_ctx *ctx, int nsteps);

/* lbm_run + device-side timing: *ms = elapsed time of the nsteps step loop measured with HIP
 * events recorded on the stream the kernels run on (max over slabs).  Synchronises. */
int lbm_run_timed(lbm_ctx *ctx, int nsteps, double *ms);

/*
 * lbm_run with timing events around every launch of the context's first slab (at most 64 launch sets are
 * recorded; run few steps).  Synchronises.  stats[8] (microseconds are means over the recorded launch sets):
 *   [0] launch sets recorded   [1] timesteps per launch set (mean)
 *   [2] edge launch us         [3] halo exchange us (from the end of the edge launch to the end of the push
 *                                  kernel / RCCL send+recv on the edge stream; the last set of a run has none)
 *   [4] interior launch us (the only launch of a context without halo rows)
 *   [5] launch-set period us (start of an interior launch to the start of the next)
 *   [6] start of the interior launch after the start of the edge launch, us   [7] transport in use
 * Diagnostic only (the events cost a few microseconds per set): bench.py --gpus N prints it per rank so that a
 * multi-GPU record explains where a launch set's time went.
 */
int lbm_run_profiled(lbm_ctx *ctx, int nsteps, double *stats);

/* Wait for all queued work.  Replaces clFinish (d2q9-bgk.c:239). */
int lbm_sync(lbm_ctx *ctx);

/*
 * Device -> host.  Replaces the two clEnqueueReadBuffer calls (d2q9-bgk.c:251-260).  Either
 * pointer may be NULL.  cells_out receives the CURRENT state whatever the step parity (the
 * reference reads a fixed buffer, correct only for even step counts).  av_vels_out receives
 * lbm_steps_done() floats.  Synchronises.  In rank mode cells_out is the GLOBAL array and only
 * this rank's rows are written; av_vels_out is the all-reduced global record — asking for it is a
 * collective operation: every rank must make the same call.  lbm_reynolds is collective in rank mode too.
 */
int lbm_download(lbm_ctx *ctx, float *cells_out, float *av_vels_out);

/* Steps applied since the last lbm_upload. */
int lbm_steps_done(const lbm_ctx *ctx);

/* Rows [*y0, *y1) of the global grid held by this context (whole grid unless rank mode). */
int lbm_row_range(const lbm_ctx *ctx, int *y0, int *y1);

/*
 * Output stage on the device: the per-cell columns of final_state.dat (d2q9-bgk.c:787-832:
 * u_x, u_y, speed u, pressure; obstacle cells give 0,0,0,density/3) and the Reynolds number of
 * the current state (av_velocity + calc_reynolds, d2q9-bgk.c:396-442,747-752).  Each output is
 * float[ny][nx] (rank mode: global array, own rows written) and may be NULL.  Synchronises.
 */
int lbm_final_state(lbm_ctx *ctx, float *u_x, float *u_y, float *u, float *pressure);
int lbm_reynolds(lbm_ctx *ctx, float *reynolds_out);

/*
 * Tuning knobs (all optional; defaults are the measured-best on MI355X):
 *   "variant"      how a thread gets its x-1/x+1 neighbours: 0 = auto, 1 = scalar L1 loads,
 *                  2 = unaligned 16-byte loads, 3 = wave64 DPP shifts, 4 = LDS-staged row with halo
 *   "fuse"         1 (or 2) = advance two timesteps per launch (intermediate state kept in registers, half
 *                  the HBM traffic), 3 = three timesteps per launch (two windows of intermediate rows, a third
 *                  of the traffic), 4 = four timesteps per launch (with row slabs only where the halo rows are 4
 *                  deep — slabs of 2M cells and more — else 3), 6..8 = the deep window kernel (lanes of two cells) with
 *                  at most that many timesteps per launch: a run is cut into the fewest launches, of equal depth
 *                  (20 steps = 7 + 7 + 6); with row slabs capped by the halo depth (8 for slabs of 3M cells and more);
 *                  falls back to 4 on grids under 32 rows per slab.  0 = one launch per step, -1 = auto (by size: 8
 *                  from 3M cells per slab; one slab without halo rows: above 300K cells, always as chunk pairs).  5 = the
 *                  chunk pairs at five steps per launch set on row slabs that carry five halo rows (slabs of 240K to 3M cells)
 *                  in compact launch sets — what auto chooses there; the four-step kernel anywhere else.
 *   "twin_steps"   chunk-pair form of the deep window kernel ("pair"): most timesteps per launch, 2..8, 0 = auto (5 below
 *                  3M cells, 8 from there on)
 *   "steady"       deep window kernel: -1/1 = a launch of exactly 5 (chunk pairs below 3M cells), 6, 7 or 8 timesteps runs the
 *                  kernel instantiated for that depth (general form of the row loop while the levels start up, then a steady
 *                  form whose level chain is straight-line code), 0 = the any-depth kernel always.  Same results bit for bit.
 *   "edge_aware"   deep window kernel with row slabs: -1/1 = one-round interior schedule whose last units take over the
 *                  wave slots of the edge launch, 0 = slots reserved for the whole launch set
 *   "obst_paths"   deep window kernel: 1 (and -1, auto) = waves that hold no blocked cell take a collision path without
 *                  the bounce-back selects, 0 = one path
 *   "balance"      deep window kernel, launches that are one round of work units: 1 (and -1, auto) = the strips that hold blocked
 *                  cells in most rows (at most four: a cavity's wall strips) are worked on by twice the waves, each on half of
 *                  every chunk of rows, so that the launch does not end with them; 0 = every strip the same.  Reads back as
 *                  the number of strips doubled.  Same results bit for bit.
 *   "free_sweeps"  deep window kernel at 6, 7, 8 timesteps per launch: 1 (and -1, auto) = a wave whose chunk of rows holds no
 *                  blocked cell inside its strip (looked up in a map built from the obstacle map) sweeps it without any
 *                  obstacle handling, 0 = every wave looks level by level ("obst_paths").  Same results bit for bit.
 *   "core_loop"    deep window kernel, free sweeps: 1 (and -1, auto) = the rows of a chunk's interior — every level on one of
 *                  the chunk's own rows, none on the accelerated row, no row wrap — run a form of the row loop without the
 *                  per-level tests and with carried row pointers, 0 = the steady form throughout.  Reads back as 0 or 1.
 *                  Same results bit for bit.
 *   "windows", "load_bufs"   kept for callers that set them: the three-step kernel exists in ONE form since round 4 — its two
 *                  windows in LDS (two waves per SIMD), one row-set of source loads in flight; "windows" accepts -1 / 1,
 *                  "load_bufs" 0 / 1 (the register-window form and the two-row-set form, 253-256 registers at one wave per
 *                  SIMD, were measured slower in rounds 1-2 and no policy selected them)
 *   "sched_waves"  waves per SIMD the three- / four-step kernels' chunk schedule plans for: 1 or 2, 0 = auto
 *   "pair"         chunk-pair form of the three- / four-step kernels and of the deep window kernel (two chunks that start
 *                  at a common boundary run as one workgroup and hand each other their first rows instead of computing
 *                  them twice): 1 = always, 0 = never, -1 = auto (where all units of a launch are resident at once; the
 *                  deep window kernel: one slab without halo rows; with row slabs the interior of a compact launch set —
 *                  peer stores — from about 650 rows per slab at 8192 cells a row)
 *   "multistep"    T = 1..8: advance T timesteps per launch on LDS-resident tiles (small, launch-bound
 *                  grids), 0 = off, -1 = auto.  Single-slab grids only; takes precedence over "fuse".
 *   "resident"     1 = run all timesteps of an lbm_run (up to 256 per launch: the ring of per-step sums) in ONE launch with the
 *                  grid held in registers (d2q9_resident: bands of 2, 4 or 6 full-width rows, one to eight waves across; neighbouring
 *                  bands trade their edge rows through memory behind step words, bounded by "halo_timeout_ms") where the grid
 *                  allows it — one slab without halo rows, nx a multiple of 4 from 128 to 1024 (a band's last wave may be partly filled), ny a
 *                  multiple of the band height, all
 *                  bands resident on the device at once (up to 1.5M cells on 256 CUs) —, 0 = never, -1 = auto: from 200K cells
 *                  while "fuse" and "multistep" are on auto.  Reads back as the rows per band in use (0 = not in use).
 *                  Bit-identical to single steps.  A band that waits in vain ends the run with LBM_ERR_COMM.  Such a launch needs
 *                  the whole device: the library orders the resident launches of all contexts of a process one behind the other;
 *                  whatever else fills the device meanwhile (another process, a long kernel of the caller's) delays it.
 *   "chunk_rows"   most rows swept by one wave of the two-step kernel (0 = auto)
 *   "chunk_min"    fewest rows per wave at the tapered end of the schedule (0 = auto)
 *   "pair_taper"   taper of a chunk-pair schedule of several rounds, in 1/32 (csrc/chunk_schedule.h): -1 = auto, 0 = size the
 *                  chunks one by one as an unpaired schedule does
 *   "grid_blocks"  cap on workgroups per launch (0 = auto)
 *   "nt_stores"    1 = non-temporal stores for the destination grid, 0 = plain, -1 = auto
 *   "nt_loads"     source loads of the two-step kernel: 0 = plain, 1 = non-temporal, 2 = non-temporal except for the rows shared
 *                  with the neighbouring chunk, -1 = auto (2).  The three- and four-step kernels always load plain (with two waves
 *                  per SIMD plain loads won at every size; the four-step kernel's non-temporal forms spilled and were removed).
 *   "transport"    halo transport of a context that carries halo rows: 1 = RCCL send/recv (needs a communicator),
 *                  3 = peer stores (needs connected peers); read-only values 2 = device-to-device copies, 0 = none yet
 *   "halo_sync"    peer transport, consumer side: 0 = wait kernel with a bounded spin (default), 1 = hipStreamWaitValue32
 *                  (UNBOUNDED: the stream waits for a neighbour that died for ever; diagnostic use), 2 = the edge tiles /
 *                  edge chunks of the consuming launch poll the flag words themselves (compact launch sets only,
 *                  elsewhere like 0; refused with LBM_ERR_STATE while a ring neighbour lives on another device or in
 *                  another process on another device — there the halo rows are read behind the wait kernel's
 *                  kernel-start acquire)
 *   "halo_timeout_ms"  bound of that spin, 1..600000 (default 30000).  ONE timeout per run: the first wait that gives up
 *                  raises the slab's error word and every later wait falls through at once, so the launch sets already
 *                  queued drain at kernel speed; lbm_sync / lbm_download then return LBM_ERR_COMM and the context
 *                  accepts only lbm_destroy
 *   "push_release" peer transport, producer side: how a pushing wave orders its halo rows before the flag words go up.  1 = release
 *                  fences at system scope around the ticket (the HSA memory model's guarantee, whatever path the stores took),
 *                  0 = write-through stores drained with s_waitcnt (measured and soak-tested between slabs and processes on ONE
 *                  device only), -1 = auto: 1 whenever a ring neighbour lives on another device.  Same results bit for bit.
 *   "debug_stale_exchange"  TEST HOOK, n >= 1: the n-th halo exchange from now announces itself (flag words, events) but
 *                  delivers no rows — on every rank of the ring alike —, 0 = off; clears itself when it fires.  Exists so that the
 *                  checks above the library (bench.py: transport_check) can be shown to catch a transport that loses halo rows.
 *   "compact"      row slabs: -1/1 = one launch per launch set on one stream, its first workgroups — the edge tiles /
 *                  edge chunks — store the halo rows into the neighbours themselves (peer transport: LDS-tile kernel, three- /
 *                  four-step kernels, deep window kernel incl. its five-step chunk pairs on slabs of 300K to 3M cells) or, under
 *                  the RCCL transport on slabs that run the deep window kernel (from 3M cells) or its five-step chunk pairs
 *                  (540K to 3M cells), into staging blocks which the edge stream sends once the flag word of the launch's last
 *                  edge wave is up (hipStreamWaitValue32: "staged" launch sets);
 *                  0 = edge launch / interior launch / push kernel (or RCCL exchange) on two streams
 * Read-only through lbm_get_option: "nslabs", "fuse_units", "halo_depth", "launch_steps" (most timesteps one launch of
 * the context's main kernel advances), "cus" (compute units of the first slab's device, which its schedules plan for).
 */
int lbm_set_option(lbm_ctx *ctx, const char *key, long value);
int lbm_get_option(const lbm_ctx *ctx, const char *key, long *value);

/* Roofline denominator: float4 device-to-device copy kernel (read bytes + written bytes per
 * second, in GB/s) on the current device; bytes is the size of each of the two buffers. */
int lbm_copy_bandwidth(size_t bytes, int iters, double *gbps);

/* The other roofline denominator, for the kernels that are bound by instruction issue (d2q9_deep): the rate at which the
 * device issues packed fp32 fused multiply-adds (eight independent chains per thread, eight waves per SIMD), in 1e12
 * lane-instructions per second, over `launches` launches of ~2 ms.  (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3.) */
int lbm_valu_rate(int launches, double *tera_lane_instr_per_s);

/*
 * Page-locked host memory for the read-back targets (the reference mallocs them in initialise(), d2q9-bgk.c:519-526,
 * outside its timed region, and frees them in finalise(), :720-727): device -> host copies of lbm_download and
 * lbm_final_state into such a buffer run at the PCIe rate (~55 GB/s) instead of the ~20 GB/s a freshly malloc'ed,
 * never-touched pageable buffer gets (every page faults inside the copy) — SURVEY 8 (f2): "so the reference-rule wall
 * time is not dominated by I/O".  Optional: every entry point takes any host pointer.  bytes > 0; lbm_host_free(NULL) is
 * a no-op.  The memory belongs to the caller until lbm_host_free; free it before the process's last lbm_destroy or after,
 * either order is valid.
 */
int lbm_host_alloc(void **ptr_out, size_t bytes);
int lbm_host_free(void *ptr);

/* Release everything.  Replaces the clRelease* block of finalise (d2q9-bgk.c:729-741). */
void lbm_destroy(lbm_ctx *ctx);

/*
 * ---- Ensembles: N independent grids of one size, advanced together ------------------------------------------------
 *
 * Grids of a few hundred cells a side (the sizes the reference ships) cannot fill the device and every launch on one of
 * them is mostly latency; they are run in numbers — a sweep over omega / accel (a Reynolds-number sweep), over obstacle
 * maps, over initial states.  An ensemble holds N such simulations ("members") on the current device, each with its own
 * run constants, obstacle map and state, and advances all of them with one launch per (up to) eight timesteps.  The members
 * never interact, and every member computes, bit for bit, the cells an ordinary context (lbm_create) computes for the same
 * inputs; its av_vels agree up to summation order.  The reference has no counterpart: one grid, one in-order queue
 * (d2q9-bgk.c:221-239); each entry point below stands beside the ordinary one of the same name and says which call sites
 * that one replaces.  Conventions as at the top of this file; one host thread drives an ensemble; arrays carry the member
 * index first: cells = float[n][9][ny][nx], obstacles = int32[n][ny][nx], fields = float[n][ny][nx].
 */
typedef struct lbm_ens lbm_ens; /* opaque */

/*
 * Create an ensemble of n members on the current HIP device (beside lbm_create: d2q9-bgk.c:600-710, and the obstacle
 * upload, :205-209).  params[n]: nx, ny and max_iters are the same in all members; reynolds_dim, density, accel, omega,
 * free_cells_inv are each member's own.  obstacles = int32[n][ny][nx], borrowed for the duration of the call.
 * Refused with LBM_ERR_ARG before any device is touched: n < 1 or n > 65535, NULL pointers, members that differ in nx, ny or
 * max_iters, a grid under 3x3, and members of more than 300 x 1024 cells — above that size a grid is no longer bound by
 * launch latency: use ordinary contexts.  An ensemble that does not fit the device's free memory is refused with LBM_ERR_HIP.
 * On failure *out is NULL.
 */
int lbm_ens_create(lbm_ens **out, const lbm_params *params, const int32_t *obstacles, int n);

/* Host -> device copy of all members' initial states, float[n][9][ny][nx] (beside lbm_upload: d2q9-bgk.c:200-203).
 * cells == NULL initialises every member's rest state from its own density on the device (d2q9-bgk.c:529-550).  Resets the
 * step counter.  Synchronises. */
int lbm_ens_upload(lbm_ens *e, const float *cells);

/* Advance every member by nsteps timesteps (accelerate_flow on row ny-2 + timestep + av_vels reduction each, per member);
 * asynchronous, repeatable (beside lbm_run: the loop body d2q9-bgk.c:221-238).  A run is cut into the fewest launches of
 * equal depth, at most 8 steps each (20 = 7 + 7 + 6).  steps_done + nsteps may not exceed max_iters (LBM_ERR_STATE). */
int lbm_ens_run(lbm_ens *e, int nsteps);

/* lbm_ens_run + device-side timing: *ms = elapsed time of the whole step loop (prologue included) measured with HIP events
 * on the stream the kernels run on (beside lbm_run_timed).  Synchronises. */
int lbm_ens_run_timed(lbm_ens *e, int nsteps, double *ms);

/* Wait for all queued work (beside lbm_sync: clFinish, d2q9-bgk.c:239). */
int lbm_ens_sync(lbm_ens *e);

/* Device -> host (beside lbm_download: d2q9-bgk.c:251-260).  cells_out = float[n][9][ny][nx], the CURRENT state whatever the
 * step parity; av_vels_out = float[n][steps_done], member m's record times its own free_cells_inv.  Either may be NULL.
 * Synchronises. */
int lbm_ens_download(lbm_ens *e, float *cells_out, float *av_vels_out);

/* Output stage per member (beside lbm_final_state / lbm_reynolds: d2q9-bgk.c:787-832, 396-442, 747-752): each field is
 * float[n][ny][nx] and may be NULL; reynolds_out = float[n].  Synchronise. */
int lbm_ens_final_state(lbm_ens *e, float *u_x, float *u_y, float *u, float *pressure);
int lbm_ens_reynolds(lbm_ens *e, float *reynolds_out);

/* Steps applied since the last lbm_ens_upload / number of members; -1 for a NULL ensemble. */
int lbm_ens_steps_done(const lbm_ens *e);
int lbm_ens_members(const lbm_ens *e);

/* Release everything (beside lbm_destroy: d2q9-bgk.c:729-741). */
void lbm_ens_destroy(lbm_ens *e);

/*
 * ---- Steady runs: every member of an ensemble to its own steady state, in one call ------------------------------------
 *
 * A sweep over omega or accel is run for each member's steady state, and the members reach theirs at very different step
 * counts.  A steady run advances an ensemble in legs of `window` steps and, after each leg, stops every member whose own
 * av_vels record has settled.  The decision is taken on the device: a stopped member's workgroups return before they touch
 * its cells, its state is never written again, and no host round trip separates the legs.  The reference has no
 * counterpart (one grid, a fixed maxIters: d2q9-bgk.c:221-239).
 *
 * Check points.  With s0 = lbm_ens_steps_done(e) at the call, a check point is a step count s = s0 + k * window, k = 1, 2,
 * ..., with s <= s0 + max_steps and s - window >= 1.  Between check points the members still active advance by `window`
 * steps exactly as lbm_ens_run(e, window) advances them: the accelerate prologue, the fewest launches of equal depth (at
 * most 8 steps each), no fused acceleration on the last launch, the partial sums reduced into the record.  If max_steps is
 * not a multiple of window the last leg is shorter and no check follows it.
 *
 * Criterion.  Let A(s) be the float that lbm_ens_download returns for the s-th step of a member,
 * (float)(av_sum[s - 1] * (double)free_cells_inv).  A member stops at check point s if
 *     fabs((double)A(s) - (double)A(s - window)) <= rel_tol * fabs((double)A(s)),
 * evaluated on the device in IEEE double with exactly these operations, the difference and the product as separate
 * statements without contraction: the host can reproduce every decision from the downloaded record.  A NaN never stops a
 * member.  A member without a free cell (A = 0 throughout) stops at its first check point.
 *
 * The host reads one word back every few legs, the count of active members, and stops enqueuing when it is 0; what a
 * member computes does not depend on that.  The call returns after a final synchronisation.
 *
 * Afterwards lbm_ens_steps_done returns the largest member count; lbm_ens_download, lbm_ens_final_state and
 * lbm_ens_reynolds return each member's own last state (the two grid arrays are double-buffered and a leg may be an odd
 * number of launches, so which array holds a member's state is the member's own from then on), and av_vels_out is
 * float[n][steps_done] with exactly 0.0f at and beyond a member's own count.  If all members ended at the same count the
 * ensemble is an ordinary one again and lbm_ens_run continues it.  Otherwise lbm_ens_run, lbm_ens_run_timed and
 * lbm_steady_run answer LBM_ERR_STATE until lbm_ens_upload, which resets counts, parities and flags.
 *
 * Limits: these two entry points take fp32 ensembles (the double-precision ensembles have their own, lbm_dsteady_run and
 * lbm_dsteady_steps, further down); the record of a step is the launch split's (a leg of 7 steps sums its tiles in another
 * order than a launch of 8, so A(s) agrees with an uninterrupted lbm_ens_run up to summation order and bit for bit with
 * lbm_ens_run(e, window) repeated); the stopped members' workgroups are still launched, and return at once.
 */

/*
 * Advance every member until ITS OWN av_vels record has settled, at most max_steps steps (beside lbm_ens_run).
 * Synchronises.  Refused with LBM_ERR_ARG before the ensemble or a device is touched: a NULL ensemble, max_steps < 0,
 * window < 1, rel_tol negative or not finite.  s0 + max_steps > max_iters, and an ensemble whose members are at different
 * counts, are answered with LBM_ERR_STATE.  max_steps == 0 is a no-op.  A failure after launches began is handled as in
 * lbm_ens_run: what was enqueued is drained, and the ensemble accepts only lbm_ens_destroy.
 */
int lbm_steady_run(lbm_ens *e, int max_steps, int window, double rel_tol);

/* Per member: steps applied since the last lbm_ens_upload, and whether it met the criterion of the last lbm_steady_run
 * since then (beside lbm_ens_steps_done).  steps_out = int[n], converged_out = int[n] (1 / 0); either may be NULL. */
int lbm_steady_steps(lbm_ens *e, int *steps_out /*[n]*/, int *converged_out /*[n]*/);

/*
 * ---- Double precision: one grid in fp64 ------------------------------------------------------------------------------
 *
 * The reference's golden files (check/SIZE.av_vels.dat, check/SIZE.final_state.dat) and the Reynolds numbers of its README come
 * from its fp64 ancestor, which held every distribution in double and parsed density, accel and omega as double.  An
 * ordinary context computes in fp32 and lands a few tenths of a percent away from those files over a full-length run; a
 * double-precision context computes in fp64 and reproduces them to print precision.  It is a family of its own beside
 * lbm_create: one grid on the current device, no row slabs, ranks or halo transports.  Each entry point stands beside the
 * ordinary one of the same name and says which call sites that one replaces.  Conventions as at the top of this file, with
 * double in place of float: cells = double[9][ny][nx], fields = double[ny][nx], obstacles = int32[ny][nx].
 */
typedef struct lbm_dparams {
  int nx;                /* cells in x */
  int ny;                /* cells in y */
  int max_iters;         /* capacity of the av_vels record (steps that can be run) */
  int reynolds_dim;      /* dimension for the Reynolds number */
  double density;        /* density per link: the fp64 literal of the parameter file, not a widened float */
  double accel;          /* density redistribution */
  double omega;          /* relaxation parameter */
  double free_cells_inv; /* 1.0 / number of non-blocked cells, in double (d2q9-bgk.c:591) */
} lbm_dparams;

typedef struct lbm_dp lbm_dp; /* opaque */

/*
 * Create a double-precision context on the current HIP device (beside lbm_create: d2q9-bgk.c:600-710, and the obstacle
 * upload, :205-209).  Any nx, ny >= 3 that fits device memory (8192 x 8192: about 9.7 GB for the two grids).  obstacles is
 * borrowed for the duration of the call.  Refused with LBM_ERR_ARG before any device is touched: NULL pointers, nx or ny
 * under 3, max_iters under 1, omega or density not finite and positive, accel not finite.  A grid that does not fit the
 * device's free memory is refused with LBM_ERR_HIP.  On failure *out is NULL.
 */
int lbm_dp_create(lbm_dp **out, const lbm_dparams *params, const int32_t *obstacles);

/* Host -> device copy of the initial state, double[9][ny][nx] (beside lbm_upload: d2q9-bgk.c:200-203).  cells == NULL
 * initialises the rest state from params.density on the device (d2q9-bgk.c:529-550).  Resets the step counter.
 * Synchronises. */
int lbm_dp_upload(lbm_dp *d, const double *cells);

/* Host -> device copy of the obstacle map, int32[ny][nx] (beside lbm_upload_obstacles: d2q9-bgk.c:205-209); same nx, ny;
 * free_cells_inv stays the caller's to keep consistent.  Resets the body map (lbm_dbody_set, "Drag of a body" further down)
 * to "every blocked cell": a body is made of the blocked cells of the map it was set on.  Synchronises. */
int lbm_dp_upload_obstacles(lbm_dp *d, const int32_t *obstacles);

/* Advance nsteps timesteps (accelerate_flow on row ny-2 + timestep + av_vels reduction each); asynchronous, repeatable
 * (beside lbm_run: the loop body d2q9-bgk.c:221-238).  steps_done + nsteps may not exceed max_iters (LBM_ERR_STATE). */
int lbm_dp_run(lbm_dp *d, int nsteps);

/* lbm_dp_run + device-side timing: *ms = elapsed time of the step loop (prologue and reductions included) measured with
 * HIP events on the stream the kernels run on (beside lbm_run_timed).  Synchronises. */
int lbm_dp_run_timed(lbm_dp *d, int nsteps, double *ms);

/* Wait for all queued work (beside lbm_sync: clFinish, d2q9-bgk.c:239). */
int lbm_dp_sync(lbm_dp *d);

/* Device -> host (beside lbm_download: d2q9-bgk.c:251-260).  cells_out = double[9][ny][nx], the CURRENT state whatever the
 * step parity; av_vels_out = double[steps_done], each step's sum of |u| over the fluid cells times free_cells_inv, in
 * double.  Either may be NULL.  Synchronises. */
int lbm_dp_download(lbm_dp *d, double *cells_out, double *av_vels_out);

/* Output stage on the device in double (beside lbm_final_state / lbm_reynolds: d2q9-bgk.c:787-832, 396-442, 747-752):
 * u_x, u_y, u, pressure, each double[ny][nx] and may be NULL, obstacle cells give 0, 0, 0, density/3; the Reynolds number
 * av_velocity * reynolds_dim / (1/6 (2/omega - 1)).  Synchronise. */
int lbm_dp_final_state(lbm_dp *d, double *u_x, double *u_y, double *u, double *pressure);
int lbm_dp_reynolds(lbm_dp *d, double *reynolds_out);

/* Steps applied since the last lbm_dp_upload; -1 for a NULL context. */
int lbm_dp_steps_done(const lbm_dp *d);

/*
 * Two options (beside lbm_set_option / lbm_get_option):
 *   "multistep"   -1 = auto (the LDS-tile form up to 300K cells, else one step per launch), 0 = one step per launch
 *                 (d2q9_dp_step), 1..8 = that many steps per launch on LDS-resident tiles (d2q9_dp_multi); a run is cut
 *                 into the fewest launches of equal depth.  Both forms give the same cells, av_vels and fields bit for bit.
 *   "force"       0 (default) | 1 = record the force on the blocked cells per step ("Drag and lift", further down:
 *                 lbm_dforce_record).  Accepted only while lbm_dp_steps_done is 0, on a fresh context or right after
 *                 lbm_dp_upload; otherwise LBM_ERR_STATE.  Turning it on allocates double[2][max_iters] on the device.
 *                 Cells, av_vels, fields and Reynolds number are the same bits with it on or off.
 * lbm_dp_get_option("multistep") reads back the steps per launch in force (0 = one step per launch).
 */
int lbm_dp_set_option(lbm_dp *d, const char *key, long value);
int lbm_dp_get_option(const lbm_dp *d, const char *key, long *value);

/* Release everything (beside lbm_destroy: d2q9-bgk.c:729-741).  NULL is a no-op. */
void lbm_dp_destroy(lbm_dp *d);

/*
 * ---- Double-precision ensembles: N independent fp64 grids of one size, advanced together ------------------------------
 *
 * The two families above composed ("dens" = double ensemble): the small grids that are run in numbers, in the precision of
 * the golden files — a Reynolds-number sweep that has to land on fp64 results.  An ensemble holds N members on the current
 * device, each with its own run constants (lbm_dparams), obstacle map and state, and advances all of them with one launch
 * per several timesteps.  The members never interact, and every member computes, bit for bit, what a double-precision
 * context (lbm_dp_create) computes for the same inputs: cells, av_vels, fields and Reynolds number.  One option ("force":
 * lbm_dforce_ens_set_option, further down), no row slabs or ranks.  The reference has no counterpart: one grid, one in-order queue (d2q9-bgk.c:221-239); each entry point below
 * stands beside the lbm_ens_ / lbm_dp_ one of the same name and says which call sites that one replaces.  Conventions as at
 * the top of this file; one host thread drives an ensemble; arrays carry the member index first: cells =
 * double[n][9][ny][nx], obstacles = int32[n][ny][nx], fields = double[n][ny][nx].
 */
typedef struct lbm_dens lbm_dens; /* opaque */

/*
 * Create a double-precision ensemble of n members on the current HIP device (beside lbm_ens_create / lbm_dp_create:
 * d2q9-bgk.c:600-710, and the obstacle upload, :205-209).  params[n]: nx, ny and max_iters are the same in all members;
 * reynolds_dim, density, accel, omega, free_cells_inv are each member's own, in double.  obstacles = int32[n][ny][nx],
 * borrowed for the duration of the call.  Refused with LBM_ERR_ARG before any device is touched: n < 1 or n > 65535, NULL
 * pointers, members that differ in nx, ny or max_iters, a grid under 3x3, max_iters under 1, a member's omega or density not
 * finite and positive or its accel not finite, and members of more than 300 x 1024 cells — up to that size a
 * double-precision context itself is bound by launch latency; above it use lbm_dp_create.  An ensemble that does not fit the
 * device's free memory is refused with LBM_ERR_HIP.  On failure *out is NULL.
 */
int lbm_dens_create(lbm_dens **out, const lbm_dparams *params, const int32_t *obstacles, int n);

/* Host -> device copy of all members' initial states, double[n][9][ny][nx] (beside lbm_ens_upload / lbm_dp_upload:
 * d2q9-bgk.c:200-203).  cells == NULL initialises every member's rest state from its own density on the device
 * (d2q9-bgk.c:529-550).  Resets the step counter.  Synchronises. */
int lbm_dens_upload(lbm_dens *e, const double *cells);

/* Advance every member by nsteps timesteps (accelerate_flow on row ny-2 + timestep + av_vels reduction each, per member);
 * asynchronous, repeatable (beside lbm_ens_run / lbm_dp_run: the loop body d2q9-bgk.c:221-238).  A run is cut into the
 * fewest launches of equal depth.  steps_done + nsteps may not exceed max_iters (LBM_ERR_STATE). */
int lbm_dens_run(lbm_dens *e, int nsteps);

/* lbm_dens_run + device-side timing: *ms = elapsed time of the whole step loop (prologue and reductions included) measured
 * with HIP events on the stream the kernels run on (beside lbm_ens_run_timed / lbm_dp_run_timed).  Synchronises. */
int lbm_dens_run_timed(lbm_dens *e, int nsteps, double *ms);

/* Wait for all queued work (beside lbm_ens_sync / lbm_dp_sync: clFinish, d2q9-bgk.c:239). */
int lbm_dens_sync(lbm_dens *e);

/* Device -> host (beside lbm_ens_download / lbm_dp_download: d2q9-bgk.c:251-260).  cells_out = double[n][9][ny][nx], the
 * CURRENT state whatever the step parity; av_vels_out = double[n][steps_done], member m's per-step sum of |u| over its fluid
 * cells times its own free_cells_inv, in double.  Either may be NULL.  Synchronises. */
int lbm_dens_download(lbm_dens *e, double *cells_out, double *av_vels_out);

/* Output stage per member on the device in double (beside lbm_ens_final_state / lbm_dp_final_state and lbm_ens_reynolds /
 * lbm_dp_reynolds: d2q9-bgk.c:787-832, 396-442, 747-752): each field is double[n][ny][nx] and may be NULL, obstacle cells
 * give 0, 0, 0, density/3; reynolds_out = double[n].  Synchronise. */
int lbm_dens_final_state(lbm_dens *e, double *u_x, double *u_y, double *u, double *pressure);
int lbm_dens_reynolds(lbm_dens *e, double *reynolds_out);

/* Steps applied since the last lbm_dens_upload / number of members; -1 for a NULL ensemble. */
int lbm_dens_steps_done(const lbm_dens *e);
int lbm_dens_members(const lbm_dens *e);

/* Release everything (beside lbm_ens_destroy / lbm_dp_destroy: d2q9-bgk.c:729-741).  NULL is a no-op. */
void lbm_dens_destroy(lbm_dens *e);

/*
 * ---- Steady runs of double-precision ensembles: every member to its own steady state, in fp64 ------------------------
 *
 * lbm_steady_run / lbm_steady_steps (above) for an lbm_dens: a Reynolds-number sweep that has to land on fp64 results is
 * run for each member's steady state, and the members reach theirs at very different step counts.  A steady run advances
 * the ensemble in legs of `window` steps and, after each leg, stops every member whose own av_vels record has settled.  The
 * decision is taken on the device: a stopped member's workgroups return before they touch its cells, its state and its
 * record beyond its count are never written again, and no host round trip separates the legs.  The reference has no
 * counterpart (one grid, a fixed maxIters: d2q9-bgk.c:221-239).
 *
 * Check points.  With s0 = lbm_dens_steps_done(e) at the call, a check point is a step count s = s0 + k * window, k = 1, 2,
 * ..., with s <= s0 + max_steps and s - window >= 1.  Between check points the members still active advance by `window`
 * steps exactly as lbm_dens_run(e, window) advances them: the accelerate prologue, the fewest launches of equal depth (at
 * most 3 steps each), no fused acceleration on the last launch, the segment sums reduced into the record.  If max_steps is
 * not a multiple of window the last leg is shorter; it is run, and no check follows it.
 *
 * Criterion, entirely in double.  Let A(s) = av_sum[s - 1] * free_cells_inv be the double that lbm_dens_download returns
 * for the s-th step of a member: the member's per-step sum times its own free_cells_inv (lbm_dparams), one multiplication.
 * A member stops at check point s if
 *     fabs(A(s) - A(s - window)) <= rel_tol * fabs(A(s)),
 * evaluated on the device in IEEE double with exactly these operations, the difference and the product as separate
 * statements without contraction: the host can reproduce every decision from the downloaded record.  A NaN never stops a
 * member; that covers a member without a free cell whose free_cells_inv is inf (0 * inf is NaN): it runs to max_steps.  A
 * member whose A is exactly 0 throughout (no free cell, a finite free_cells_inv) stops at its first check point.
 *
 * Bit identity.  A step's segment sums are added in one fixed order that does not depend on the depth of the launch that
 * computed it, so, unlike an fp32 steady run, the record does not depend on how the legs cut the launches: a member that
 * stopped at count c holds the same bits as a double-precision context (lbm_dp_*), or as a plain lbm_dens ensemble,
 * advanced to c by one run of c steps — cells, av_vels[0..c), the four fields and the Reynolds number.
 *
 * The host reads one word back every few legs, the count of active members, and stops enqueuing when it is 0; what a
 * member computes does not depend on that.  The call returns after a final synchronisation.
 *
 * Afterwards lbm_dens_steps_done returns the largest member count; lbm_dens_download, lbm_dens_final_state and
 * lbm_dens_reynolds return each member's own last state (the two grid arrays are double-buffered and a leg may be an odd
 * number of launches, so which array holds a member's state is the member's own from then on), and av_vels_out is
 * double[n][steps_done] with exactly +0.0 at and beyond a member's own count.  If all members ended at the same count the
 * ensemble is an ordinary one again, on the parity read back from the device, and lbm_dens_run continues it.  Otherwise
 * lbm_dens_run, lbm_dens_run_timed and lbm_dsteady_run answer LBM_ERR_STATE until lbm_dens_upload, which resets counts,
 * parities and flags.
 *
 * Limits: the stopped members' workgroups are still launched, and return at once.
 */

/*
 * Advance every member until ITS OWN av_vels record has settled, at most max_steps steps (beside lbm_steady_run /
 * lbm_dens_run).  Synchronises.  Refused with LBM_ERR_ARG before the ensemble or a device is touched: a NULL ensemble,
 * max_steps < 0, window < 1, rel_tol negative or not finite (the message names the argument).  s0 + max_steps > max_iters,
 * and an ensemble whose members are at different counts, are answered with LBM_ERR_STATE.  max_steps == 0 is a no-op.  A
 * failure after launches began is handled as in lbm_dens_run: what was enqueued is drained, and the ensemble accepts only
 * lbm_dens_destroy.
 */
int lbm_dsteady_run(lbm_dens *e, int max_steps, int window, double rel_tol);

/* Per member: steps applied since the last lbm_dens_upload, and whether it met the criterion of the last lbm_dsteady_run
 * since then (beside lbm_steady_steps).  steps_out = int[n], converged_out = int[n] (1 / 0); either may be NULL. */
int lbm_dsteady_steps(lbm_dens *e, int *steps_out /*[n]*/, int *converged_out /*[n]*/);

/*
 * ---- Drag and lift: the momentum-exchange force on the blocked cells, in the double-precision families -----------------
 *
 * What a sweep over omega / accel or over obstacle maps is run for is the force the flow exerts on the solid cells: drag and
 * lift, drag against Reynolds number at steady state, the lift signal of an unsteady wake.  The reference's timestep is a
 * gather followed by full-way bounce-back (kernels.cl:69, 104-112, 187-197): a blocked cell keeps what streamed into it and
 * hands it back reversed in the next step, so the momentum the solid cells take from the fluid in one step is a closed sum
 * over the solid-fluid links of values the step kernels already hold.  The reference has no counterpart (it writes av_vels
 * and the final state only, d2q9-bgk.c:241-263).
 *
 * Definition.  Speeds and their vectors c_k as at the top of this file (1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE), opp(k)
 * the opposite speed.  Let f be the state that a step streams: the state AFTER accelerate_flow for that step.  For every
 * blocked cell o and every k = 1..8 whose neighbour x = o - c_k (periodic wrap in x and y) is fluid, the link term is
 *     s = f_k(x) + f_opp(k)(o)        one addition, contraction off
 *     F += c_k * s                    i.e. +-s into F_x and / or F_y, k in ascending order within a cell
 * f_k(x) is what o gathers in that step, f_opp(k)(o) is o's own stored value, which x gathers in the same step.  Links
 * between two blocked cells do not count.  A grid without blocked cells, or without fluid cells, gives exactly +0.0.
 * F[t], t 0-based like av_vels, is this sum for step t, in lattice units per step, not divided by anything.
 *
 * Order of summation, fixed as for av_vels: a cell's eight terms in order of k; the cells of a 16-cell row segment in the
 * segment tree; the segments of a step by the second reduction stage in its order.  Hence the record is bit-identical between
 * the kernel forms ("multistep"), between launch splits, between runs, and between a double-precision context and a member
 * of a double-precision ensemble on the same inputs; and the output stage (lbm_dforce, lbm_dforce_ens) returns, bit for bit,
 * the record entry the next step writes.
 *
 * Names: lbm_dforce_* beside lbm_dsteady_*, on both double-precision handles.  The record is switched on by the option
 * "force" (lbm_dp_set_option; lbm_dforce_ens_set_option for an ensemble) before the first step; the output stage needs no
 * option.
 *
 * Out of scope: fp32 contexts and fp32 ensembles (ten kernel families, row slabs, ranks) have no force.
 */

/* The force record of a double-precision context: fx_out, fy_out = double[lbm_dp_steps_done], either may be NULL (not both:
 * LBM_ERR_ARG).  LBM_ERR_STATE if the option "force" is off.  Synchronises. */
int lbm_dforce_record(lbm_dp *d, double *fx_out, double *fy_out);

/* Output stage (beside lbm_dp_reynolds): F of the CURRENT state as the next step would stream it — accelerate_flow of row
 * ny-2 is applied on the fly, the state is not modified.  Works whether or not "force" is on.  Either pointer may be NULL
 * (not both: LBM_ERR_ARG).  Synchronises. */
int lbm_dforce(lbm_dp *d, double *fx, double *fy);

/*
 * The options of a double-precision ensemble (beside lbm_dp_set_option / lbm_dp_get_option); one key:
 *   "force"       0 (default) | 1 = record every member's force per step.  Accepted only while lbm_dens_steps_done is 0, on
 *                 a fresh ensemble or right after lbm_dens_upload; otherwise LBM_ERR_STATE.  Turning it on allocates
 *                 double[2][n][max_iters] on the device.  Cells, av_vels, fields and Reynolds numbers are the same bits with
 *                 it on or off; a steady run (lbm_dsteady_run) records the force of every member while it is active.
 * Unknown keys, NULL arguments: LBM_ERR_ARG.
 */
int lbm_dforce_ens_set_option(lbm_dens *e, const char *key, long value);
int lbm_dforce_ens_get_option(const lbm_dens *e, const char *key, long *value);

/* The force records of all members: fx_out, fy_out = double[n][lbm_dens_steps_done], either may be NULL (not both:
 * LBM_ERR_ARG).  After a steady run exactly +0.0 at and beyond a member's own count, as av_vels.  LBM_ERR_STATE if the option
 * "force" is off.  Synchronises. */
int lbm_dforce_ens_record(lbm_dens *e, double *fx_out /*[n][steps]*/, double *fy_out /*[n][steps]*/);

/* Output stage per member (beside lbm_dens_reynolds): lbm_dforce for every member, fx, fy = double[n], either may be NULL
 * (not both).  After a steady run each member's own last state is read, from the grid array that holds it.  Synchronises. */
int lbm_dforce_ens(lbm_dens *e, double *fx /*[n]*/, double *fy /*[n]*/);

/*
 * ---- Drag of a body: the force on chosen blocked cells, and steady runs that stop on it ----------------------------------
 *
 * The inputs drag sweeps run on are walled channels with a body in them, and the force above counts the walls with the body.
 * A body map says which blocked cells count: int32[ny][nx] (int32[n][ny][nx] for an ensemble), non-zero = "this blocked
 * cell's links count".
 *
 * Semantics.  With a body map the definition of "Drag and lift" is unchanged except that the outer sum runs over the blocked
 * cells of the body only.  A link still counts only if the neighbour o - c_k is fluid: a blocked neighbour, in the body or
 * not, gives no link.  No body map is the default: every blocked cell counts.  A body map with no cell set gives exactly +0.0
 * in both components.  A body map that selects every blocked cell gives the bits that no body map gives.  A non-zero entry
 * on a fluid cell is refused with LBM_ERR_ARG, the message names the first such cell (member, y, x), and nothing on the device
 * changes.
 *
 * Nothing else moves.  Cells, av_vels, the four fields and Reynolds numbers are the same bits with any body map as with none:
 * a blocked cell outside the body is a blocked cell to collision, acceleration and the output stages.  The record with a
 * body keeps every bit identity stated under "Drag and lift" (kernel forms, launch splits, runs, context and ensemble
 * member, steady-run member and plain run), and the output stage equals the record entry the next step writes.  The caller
 * never sees how the device tells the two kinds of blocked cell apart: lbm_dbody_get returns 0 and 1 only.
 *
 * When a map is accepted.  With the option "force" off: at any time; the output stage (lbm_dforce, lbm_dforce_ens) reads the
 * body in force at the call, so the forces of several bodies on one state are several set + force calls.  With "force" on:
 * only while steps_done is 0, the rule of the option itself; otherwise LBM_ERR_STATE, so one record never mixes two bodies
 * (that includes an ensemble left ragged by a steady run: its counts are not 0).  lbm_dp_upload_obstacles resets the body
 * to "every blocked cell"; lbm_dp_upload and lbm_dens_upload keep it.  Setting a map rewrites the device mask from the host's
 * copy of the obstacle map and synchronises.
 *
 * Drag criterion.  lbm_dbody_steady_run is lbm_dsteady_run in everything but the criterion: the legs, check points, polling,
 * gating, lbm_dsteady_steps for the per-member counts, raggedness, what downloads return afterwards, argument refusals and
 * the failure latch are that entry point's.  Let F(s) be the F_x record entry of the member's s-th step, fx_out[m][s - 1] as
 * lbm_dforce_ens_record returns it; nothing is multiplied into it.  A member stops at check point s if
 *     fabs(F(s) - F(s - window)) <= rel_tol * fabs(F(s)),
 * evaluated on the device in IEEE double, the difference and the product as separate statements without contraction: the
 * host reproduces every decision from the downloaded record.  A NaN never stops a member.  A member whose F_x is exactly 0
 * throughout (an empty body, or no blocked cell) stops at its first check point.
 *
 * Out of scope here: more than one body per record (the output stage with the record off covers several bodies on one
 * state), drag and lift coefficients (the reference velocity and length are the caller's), a combined av_vels-and-drag
 * criterion.
 */

/* Set the body map of a double-precision context, int32[ny][nx], borrowed for the call; NULL: every blocked cell counts
 * again.  LBM_ERR_ARG: a NULL context, a non-zero entry on a fluid cell.  LBM_ERR_STATE: "force" on and steps done.
 * Synchronises. */
int lbm_dbody_set(lbm_dp *d, const int32_t *body);

/* body_out = int32[ny][nx]: 1 where a blocked cell counts, else 0.  A NULL context or a NULL body_out: LBM_ERR_ARG. */
int lbm_dbody_get(lbm_dp *d, int32_t *body_out);

/* The same for all members of a double-precision ensemble, int32[n][ny][nx]. */
int lbm_dbody_ens_set(lbm_dens *e, const int32_t *body);
int lbm_dbody_ens_get(lbm_dens *e, int32_t *body_out);

/*
 * Advance every member until ITS OWN drag has settled, at most max_steps steps (beside lbm_dsteady_run, whose refusals it
 * shares).  The option "force" must be on: otherwise LBM_ERR_STATE, and the message says to switch it on before the first
 * step.  Synchronises.
 */
int lbm_dbody_steady_run(lbm_dens *e, int max_steps, int window, double rel_tol);

/*
 * ---- Two relaxation times: a second collision operator for the double-precision families -------------------------------
 *
 * A drag-against-Reynolds-number sweep is a sweep over omega, and with BGK and bounce-back the plane where a wall
 * effectively sits moves with the relaxation rate: every member of the sweep sees a slightly different body in a slightly
 * different channel, an error in the drag curve that no step count removes.  The two-relaxation-time (TRT) operator relaxes
 * the symmetric part of each pair of opposite populations with omega, which sets the viscosity, and the antisymmetric part
 * with a second rate omega_m, tied to omega by the magic parameter
 *     Lambda = (1/omega - 1/2) (1/omega_m - 1/2).
 * At fixed Lambda the wall location does not depend on the viscosity: Lambda = 3/16 puts a straight wall exactly half-way
 * between the blocked cell and its fluid neighbour, Lambda = 1/4 is the most stable choice.  Off by default: BGK, the
 * reference's operator (kernels.cl:119-198), keeps every bit.  The reference has no counterpart.
 *
 * Definition.  The host computes omega_m in double, three separate statements without contraction:
 *     tp = 1.0 / omega - 0.5;
 *     tm = magic / tp + 0.5;
 *     omega_m = 1.0 / tm;
 * A fluid cell's density, momentum, u_sq and equilibrium eq[0..8] from its gathered values g[0..8] are the BGK statements,
 * unchanged, and so are the |u| it adds to av_vels and the bounce-back of a blocked cell.  Only the relaxation lines differ,
 * contraction off:
 *     out[0] = g[0] + omega * (eq[0] - g[0]);
 *     for (k, q) in (1,3), (2,4), (5,7), (6,8):
 *         a  = eq[k] - g[k];      b  = eq[q] - g[q];
 *         sp = 0.5 * (a + b);     sm = 0.5 * (a - b);
 *         rp = omega * sp;        rm = omega_m * sm;
 *         out[k] = g[k] + (rp + rm);
 *         out[q] = g[q] + (rp - rm);
 * Lambda = 1/4 at omega = 1 gives omega_m = 1 exactly; that TRT step rounds five more times per value than the BGK step and is
 * not promised its bits, only to stay within those roundings of it.
 *
 * Nothing else moves: accelerate_flow, bounce-back, the momentum-exchange force and its body maps, the order of every sum,
 * the four fields, and the Reynolds number, whose viscosity still comes from omega.  Every bit identity stated for BGK holds
 * for TRT: between the kernel forms ("multistep"), launch splits and runs; between a double-precision context and a member
 * of a double-precision ensemble with the same magic parameter; between a member stopped by lbm_dsteady_run or
 * lbm_dbody_steady_run at count c and a plain run of c steps.  Both steady runs work with TRT unchanged.
 *
 * When it is accepted.  Only while steps_done is 0, on a fresh handle or right after an upload, the rule of the option
 * "force": otherwise LBM_ERR_STATE.  lbm_dp_upload, lbm_dens_upload and lbm_dp_upload_obstacles keep the setting.  An ensemble
 * runs either all members TRT, each with its own magic parameter, or all BGK.
 *
 * Names: lbm_dtrt_*, on both double-precision handles (the option entry points take a long, which cannot carry 3/16).
 * Out of scope: fp32 contexts and fp32 ensembles, whose checker contract is the reference's BGK.
 */

/* Set the collision operator of a double-precision context: magic == 0.0 is BGK (the default), magic > 0 and finite is TRT
 * with that magic parameter.  LBM_ERR_ARG, before the context is read: a NULL context, magic negative, NaN or infinite.
 * LBM_ERR_ARG: magic > 0 on a context whose 1/omega - 1/2 <= 0, that is omega >= 2 (the message names omega).
 * LBM_ERR_STATE: steps done. */
int lbm_dtrt_set(lbm_dp *d, double magic);

/* The magic parameter in force (0.0: BGK) and the second relaxation rate, which is omega itself under BGK.  Either output may
 * be NULL; both NULL (magic_out and omega_minus_out), or a NULL context: LBM_ERR_ARG. */
int lbm_dtrt_get(const lbm_dp *d, double *magic_out, double *omega_minus_out);

/* The same for a double-precision ensemble: magic = double[n], every entry > 0 and finite, members may differ; NULL: all
 * members BGK.  LBM_ERR_ARG, the message names the member: an entry that is 0, negative, NaN or infinite, a member whose
 * omega >= 2; nothing on the device changes after a refusal.  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_dtrt_ens_set(lbm_dens *e, const double *magic /*[n]*/);
int lbm_dtrt_ens_get(const lbm_dens *e, double *magic_out /*[n]*/, double *omega_minus_out /*[n]*/);

/*
 * ---- Open boundaries: velocity inlet and pressure outlet for the double-precision families ------------------------------
 *
 * Every double-precision grid is periodic in x and y, and the flow is driven by accelerate_flow on the row ny - 2: a body in
 * such a channel stands in its own wake, which re-enters from the left, and nothing defines a free-stream velocity or a drag
 * coefficient.  With open boundaries the fluid cells of column 0 carry a prescribed velocity profile (u_in[y], 0) and the
 * fluid cells of column nx - 1 a prescribed density rho_out, both by the Zou-He construction: the populations that entered
 * across the x wrap are replaced by the non-equilibrium bounce-back of their opposites plus what the prescribed moment asks
 * for.  Off by default: the periodic, accelerated flow of the reference (kernels.cl:9-53, 56-231) keeps every bit.  The
 * reference has no counterpart.
 *
 * Definition.  With open boundaries on, a step is gather, boundary fix, collision.
 *   Gather.  Unchanged: g[k](x) = f_k(x - c_k), periodic wrap in x and y.
 *   No accelerate_flow.  It is not applied anywhere: not as the prologue of a run, not fused into a step, not in the output
 *   stage of the force (lbm_dforce, lbm_dforce_ens).  `accel` in the params is ignored while the setting is on.
 *   Boundary fix.  It replaces three gathered values of every FLUID cell of column 0 and of column nx - 1, before the collision
 *   (BGK or TRT, as set).  Blocked cells are untouched and bounce back what they gathered.  All in double, contraction off,
 *   one IEEE operation per written operator, in this order; 2.0 / 3.0 and 1.0 / 6.0 are double constants.
 * Inlet, x == 0, fluid, u = u_in[y]:
 *     s0 = (g[0] + g[2]) + g[4];      s1 = (g[3] + g[6]) + g[7];
 *     rho = (s0 + 2.0 * s1) / (1.0 - u);
 *     ru = rho * u;                   d = 0.5 * (g[2] - g[4]);
 *     g[1] = g[3] + (2.0 / 3.0) * ru;
 *     g[5] = (g[7] - d) + (1.0 / 6.0) * ru;
 *     g[8] = (g[6] + d) + (1.0 / 6.0) * ru;
 * Outlet, x == nx - 1, fluid, rho_out:
 *     s0 = (g[0] + g[2]) + g[4];      s1 = (g[1] + g[5]) + g[8];
 *     ru = (s0 + 2.0 * s1) - rho_out; d = 0.5 * (g[2] - g[4]);
 *     g[3] = g[1] - (2.0 / 3.0) * ru;
 *     g[7] = (g[5] + d) - (1.0 / 6.0) * ru;
 *     g[6] = (g[8] - d) - (1.0 / 6.0) * ru;
 * nx >= 3 holds for every grid, so the two columns are distinct.  Every population that crosses the x wrap into a fluid cell is
 * one of the six replaced: the fluid is decoupled across the wrap.  The y wrap stays; the channels have walls there.
 *
 * Force.  The per-cell definition of "Drag and lift" and the order of every sum are unchanged.  One rule is added: while open
 * boundaries are on, the blocked cells of columns 0 and nx - 1 count as outside every body (with or without a body map), so
 * that no link across the x wrap enters a force.  lbm_dbody_get still returns the caller's body.
 *
 * Nothing else moves: av_vels, the four fields and the Reynolds number keep their definitions, and every bit identity stated
 * for the periodic flow holds with open boundaries: between the kernel forms ("multistep"), launch splits and runs; between a
 * double-precision context and a member of a double-precision ensemble with the same profile and rho_out; between a member
 * stopped by lbm_dsteady_run or lbm_dbody_steady_run at count c and a plain run of c steps.  It composes with "force", body
 * maps and TRT.
 *
 * When it is accepted.  Only while steps_done is 0, the rule of the option "force" and of lbm_dtrt_set: otherwise
 * LBM_ERR_STATE.  lbm_dp_upload, lbm_dens_upload and lbm_dp_upload_obstacles keep the setting; the obstacle upload rewrites
 * the device mask under the column rule above.  An ensemble is all open or all periodic; members differ in profile and
 * rho_out.  After a refusal nothing has changed, on the host or on the device.
 *
 * Names: lbm_dopen_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, whose checker
 * contract is the reference's periodic flow.
 */

/* Open boundaries of a double-precision context: u_in = double[ny], borrowed for the call, the inlet velocity of every row
 * (entries on rows whose column-0 cell is blocked are not read by any kernel but are checked like the others); rho_out the
 * outlet density.  u_in == NULL: off (the default), rho_out is not read.  LBM_ERR_ARG: a NULL context; rho_out not finite and
 * positive; a u_in entry that is not finite or is >= 1 (the message names the row).  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_dopen_set(lbm_dp *d, const double *u_in /*[ny]*/, double rho_out);

/* on_out: 1 while open boundaries are on, else 0; while they are on, u_in_out = double[ny] and rho_out_out get the setting,
 * while they are off neither is written.  Any output may be NULL; all three NULL (on_out, u_in_out and rho_out_out), or a NULL
 * context: LBM_ERR_ARG. */
int lbm_dopen_get(const lbm_dp *d, int *on_out, double *u_in_out /*[ny]*/, double *rho_out_out);

/* The same for all members of a double-precision ensemble: u_in = double[n][ny], rho_out = double[n]; u_in == NULL: off.
 * Everything is checked before anything changes, then copied once; the message names the member and the row.  A NULL rho_out
 * beside a non-NULL u_in: LBM_ERR_ARG. */
int lbm_dopen_ens_set(lbm_dens *e, const double *u_in /*[n][ny]*/, const double *rho_out /*[n]*/);
int lbm_dopen_ens_get(const lbm_dens *e, int *on_out, double *u_in_out /*[n][ny]*/, double *rho_out_out /*[n]*/);

/*
 * ---- Moving walls: velocity bounce-back for the double-precision families ------------------------------------------------
 *
 * Every blocked cell of a double-precision grid stands still: a channel is driven by accelerate_flow or by an inlet, never by
 * a wall, so neither Couette flow nor a lid-driven cavity can be run, and the disc of "Drag of a body" cannot spin.  With
 * moving walls a blocked cell may carry a wall velocity (u_x, u_y); a context carries one wall density rho_wall, each member
 * of an ensemble its own.  What such a cell bounces back gains the momentum the wall gives the fluid, 6 w_k rho_wall c_k . u_wall
 * on speed k.  Off by default: walls at rest, the reference's bounce-back (kernels.cl:69, 187-197), keep every bit.  The
 * reference has no counterpart.
 *
 * Definition.  A blocked cell whose two components both compare equal to 0.0 is a resting wall: the existing bounce-back,
 * no arithmetic, so signed zeros survive and a map of zeros (of either sign) is the flow without the setting, bit for bit.
 * Any other blocked cell writes, from its gathered values g[0..8], the following instead of the plain swap.  All in double,
 * contraction off, one IEEE operation per written operator, in this order; 2.0 / 3.0 and 1.0 / 6.0 are double constants.
 * Moving wall, blocked, (u_x, u_y) != (0, 0):
 *     rx = rho_wall * u_x;            ry = rho_wall * u_y;
 *     a  = (2.0 / 3.0) * rx;          b  = (2.0 / 3.0) * ry;
 *     p  = (1.0 / 6.0) * (rx + ry);   q  = (1.0 / 6.0) * (ry - rx);
 *     out[0] = g[0];
 *     out[1] = g[3] + a;   out[3] = g[1] - a;
 *     out[2] = g[4] + b;   out[4] = g[2] - b;
 *     out[5] = g[7] + p;   out[7] = g[5] - p;
 *     out[6] = g[8] + q;   out[8] = g[6] - q;
 * The cell still returns |u| = 0.  Fluid cells are untouched: accelerate_flow, the open columns and TRT act on them alone.
 *
 * Nothing else moves: av_vels, the four fields (a moving cell reads 0, 0, 0, density / 3 like every blocked cell), the Reynolds
 * number, the force definition and the order of its sums, the body rules including the open-column rule, accelerate_flow, and
 * both steady criteria are unchanged.  The force needs no new term: the stored value own[opp] of a link already carries what
 * the wall added, so the momentum-exchange sum of "Drag and lift" is Ladd's sum for a moving wall.
 *
 * Mass.  A wall velocity along the wall conserves mass.  One with a component normal to the fluid adds or removes mass every
 * step; that is the caller's business, nothing checks it.
 *
 * Every bit identity stated for the existing flow holds with walls moving: between the kernel forms ("multistep"), launch
 * splits and runs; between a double-precision context and a member of a double-precision ensemble with the same velocities
 * and rho_wall; between a member stopped by lbm_dsteady_run or lbm_dbody_steady_run at count c and a plain run of c steps.
 * It composes with "force", body maps, TRT and open boundaries.
 *
 * When it is accepted.  Only while steps_done is 0, the rule of lbm_dopen_set: otherwise LBM_ERR_STATE.  lbm_dp_upload,
 * lbm_dens_upload and lbm_dp_upload_obstacles keep the setting; a velocity is read only while its cell is blocked.  An ensemble
 * has the setting on or off for all members; members differ in velocities and rho_wall.  Everything is checked before anything
 * changes: after a refusal nothing has changed, on the host or on the device.
 *
 * Names: lbm_dwall_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, whose checker
 * contract is the reference's resting walls.
 */

/* Wall velocities of a double-precision context: u_x, u_y = double[ny][nx], borrowed for the call; rho_wall the wall density.
 * u_x == NULL and u_y == NULL: off (the default), rho_wall is not read.  LBM_ERR_ARG: a NULL context; exactly one of u_x and
 * u_y NULL; rho_wall not finite and positive; an entry that is not finite; a non-zero entry on a fluid cell, as lbm_dbody_set
 * refuses a body there (the message names the cell).  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_dwall_set(lbm_dp *d, const double *u_x /*[ny][nx]*/, const double *u_y /*[ny][nx]*/, double rho_wall);

/* on_out: 1 while wall velocities are on, else 0; while they are on, u_x_out, u_y_out = double[ny][nx] and rho_wall_out get
 * the setting, while they are off none is written.  Any output may be NULL; all four NULL (on_out, u_x_out, u_y_out and
 * rho_wall_out), or a NULL context: LBM_ERR_ARG. */
int lbm_dwall_get(const lbm_dp *d, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out);

/* The same for all members of a double-precision ensemble: u_x, u_y = double[n][ny][nx], rho_wall = double[n]; u_x == NULL and
 * u_y == NULL: off.  Everything is checked before anything changes, then copied once; the message names the member and the
 * cell.  A NULL rho_wall beside non-NULL velocities: LBM_ERR_ARG. */
int lbm_dwall_ens_set(lbm_dens *e, const double *u_x /*[n][ny][nx]*/, const double *u_y, const double *rho_wall /*[n]*/);
int lbm_dwall_ens_get(const lbm_dens *e, int *on_out, double *u_x_out, double *u_y_out, double *rho_wall_out /*[n]*/);

/*
 * ---- Subgrid viscosity: the Smagorinsky model for the double-precision families ---------------------------------------------
 *
 * Every run so far is laminar: the relaxation rate is one constant per grid, and as omega approaches 2, which is what a high
 * Reynolds number on an affordable grid means, BGK and TRT with bounce-back go unstable (a 32 x 32 lid-driven cavity at omega =
 * 1.99 and lid speed 0.1 is non-finite after a few hundred steps).  With the Smagorinsky subgrid model (Hou et al. 1996) a cell
 * relaxes with its own rate: the eddy viscosity nu_t = (c Delta)^2 |S| comes from the non-equilibrium momentum flux the cell
 * already holds, so the model is local and a pure change of the collision.  Off by default: one rate per grid keeps every bit.
 * The reference has no counterpart.
 *
 * Definition.  The host computes two constants per context or member from omega and the Smagorinsky constant c, in double,
 * separate statements without contraction; sqrt(2.0) is the correctly rounded double, and the factor follows from nu_t =
 * (c Delta)^2 |S| with c_s^2 = 1/3:
 *     tau0  = 1.0 / omega;
 *     les_k = (18.0 * sqrt(2.0)) * (c * c);
 * A fluid cell, after the gather and after the boundary fix where open boundaries are on, forms its rate from its gathered values
 * g[0..8] and the moments the collision forms anyway: dens, densinv = 1.0 / dens and the momenta u_x, u_y (the BGK statements,
 * unchanged).  All in double, contraction off, one IEEE operation per written operator, in this order; 1.0 / 3.0 is a double
 * constant and sqrt is the correctly rounded square root:
 *     d57 = g[5] + g[7];  d68 = g[6] + g[8];  dgs = d57 + d68;
 *     p   = dens * (1.0 / 3.0);
 *     pxx = ((g[1] + g[3]) + dgs) - (p + (u_x * u_x) * densinv);
 *     pyy = ((g[2] + g[4]) + dgs) - (p + (u_y * u_y) * densinv);
 *     pxy = (d57 - d68) - (u_x * u_y) * densinv;
 *     q   = sqrt((pxx * pxx + pyy * pyy) + 2.0 * (pxy * pxy));
 *     tau = 0.5 * (tau0 + sqrt(tau0 * tau0 + les_k * (q * densinv)));
 *     om  = 1.0 / tau;
 * The second moment of the equilibrium is analytic, so the stress needs no eq[k] - g[k].  BGK: the relaxation lines read om where
 * they read omega.  TRT: rp = om * sp, out[0] uses om, and the second rate is recomputed per cell from the magic parameter by the
 * three statements of "Two relaxation times" with tp = tau - 0.5 in place of 1.0 / omega - 0.5:
 *     tp = tau - 0.5;
 *     tm = magic / tp + 0.5;
 *     omega_m = 1.0 / tm;
 * A cell with q == 0 gets om = 1.0 / (1.0 / omega), which is not omega to the bit: with any c > 0 the model is promised BGK's
 * bits nowhere; only c == 0.0, which is off, is.
 *
 * Nothing else moves: accelerate_flow, bounce-back and moving walls, the force and its body maps, the order of every sum, the
 * four fields, the Reynolds number, whose viscosity stays the molecular one from omega, and both steady runs.  Every bit identity
 * stated for the existing flow holds with the model on: between the kernel forms ("multistep"), launch splits and runs; between a
 * double-precision context and a member of a double-precision ensemble with the same c; between a member stopped by
 * lbm_dsteady_run or lbm_dbody_steady_run at count c and a plain run of c steps.  It composes with "force", body maps, TRT, open
 * boundaries and moving walls; it and TRT may be set in either order.
 *
 * When it is accepted.  Only while steps_done is 0, the rule of lbm_dtrt_set: otherwise LBM_ERR_STATE.  lbm_dp_upload,
 * lbm_dens_upload and lbm_dp_upload_obstacles keep the setting.  An ensemble has the model on for all members, each with its
 * own c, or off.  Everything is checked before anything changes: after a refusal nothing has changed, on the host or on the
 * device.
 *
 * Names: lbm_dles_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, which get nothing; a
 * downloadable field of the eddy viscosity; wall damping of c; any other subgrid model.
 */

/* Set the subgrid model of a double-precision context: c == 0.0 is off (the default), c > 0 and finite is on with that Smagorinsky
 * constant.  LBM_ERR_ARG, before the context is read: a NULL context, c negative, NaN or infinite.  LBM_ERR_STATE: steps done. */
int lbm_dles_set(lbm_dp *d, double c);

/* The Smagorinsky constant in force (0.0: off) and les_k as the host statements give it.  Either output may be NULL; both NULL
 * (c_out and les_k_out), or a NULL context: LBM_ERR_ARG. */
int lbm_dles_get(const lbm_dp *d, double *c_out, double *les_k_out);

/* The same for a double-precision ensemble: c = double[n], every entry > 0 and finite, members may differ; NULL: off for all
 * members.  LBM_ERR_ARG, the message names the member: an entry that is 0, negative, NaN or infinite; nothing on the device
 * changes after a refusal.  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_dles_ens_set(lbm_dens *e, const double *c /*[n]*/);
int lbm_dles_ens_get(const lbm_dens *e, double *c_out /*[n]*/, double *les_k_out /*[n]*/);

/*
 * ---- Body force: a uniform driving force by Guo forcing, for the double-precision families ------------------------------------
 *
 * Two things set a double-precision flow moving so far: accelerate_flow, which nudges three populations on the one row ny - 2
 * where a guard allows it, a first-order trick without a continuum meaning, and a velocity inlet.  A channel driven by a
 * pressure gradient, gravity in a closed box, a permeability sweep with one force per member cannot be run.  With a body force a
 * context, or each member of an ensemble, carries a constant force density F = (F_x, F_y) per cell volume; it is NOT multiplied
 * by the cell's density (the convention of the reference's density * accel constants, kernels.cl:14-15).  Every fluid cell takes
 * it up by Guo's scheme (Guo, Zheng, Shi 2002): the momenta the collision reads are shifted by half the force, and the
 * relaxation lines gain a source whose even and odd parts relax with the two rates of the collision.  Off by default: (0, 0)
 * keeps every bit.  The reference has no counterpart.
 *
 * Definition.  With the force on, every FLUID cell does the following after the gather and after the boundary fix where open
 * boundaries are on.  All in double, contraction off, one IEEE operation per written operator, in this order; w[0] = 4.0 / 9.0,
 * w[1..4] = 1.0 / 9.0, w[5..8] = 1.0 / 36.0, s[1..4] = 1.0 / 3.0 and s[5..8] = 1.0 / 12.0 (three times w) are double constants.
 * dens and densinv are the BGK statements, unchanged.  The momenta gain half the force:
 *     u_x = ((g[1] - g[3]) + (diag_a + diag_b)) + 0.5 * F_x;
 *     u_y = ((g[2] - g[4]) + (diag_a - diag_b)) + 0.5 * F_y;
 * with diag_a = g[5] - g[7] and diag_b = g[8] - g[6] as in the BGK statements.  Everything downstream reads these shifted
 * momenta: the statements of "Subgrid viscosity" where the model is on, u_sq, uvec[k], the equilibrium eq[k], and the
 * |u| = sqrt(u_sq) * densinv the cell adds to av_vels.  The source, with cF[k] = c_k . F formed in the pattern of uvec[k]
 * (cF[1] = F_x, cF[2] = F_y, cF[3] = -F_x, cF[4] = -F_y, cF[5] = F_x + F_y, cF[6] = -F_x + F_y, cF[7] = -F_x - F_y,
 * cF[8] = F_x - F_y):
 *     v_x = u_x * densinv;            v_y = u_y * densinv;
 *     uF = v_x * F_x + v_y * F_y;     t3 = 3.0 * uF;
 *     se[0] = w[0] * (0.0 - t3);
 *     for k = 1..8:
 *         cv = uvec[k] * densinv;
 *         se[k] = w[k] * (9.0 * (cv * cF[k]) - t3);
 *         so[k] = s[k] * cF[k];
 * se is the even part (the same bits on the two speeds of a pair), so the odd part (so[q] = -so[k] on the opposite speed q).
 * The relaxation lines, with pe = 1.0 - 0.5 * omega:
 *     BGK:  out[0] = (g[0] + omega * (eq[0] - g[0])) + pe * se[0];
 *           out[k] = (g[k] + omega * (eq[k] - g[k])) + pe * (se[k] + so[k]);          k = 1..8
 *     TRT:  out[0] as under BGK, and with po = 1.0 - 0.5 * omega_m, for (k, q) in (1,3), (2,4), (5,7), (6,8):
 *           fe = pe * se[k];          fo = po * so[k];
 *           out[k] = (g[k] + (rp + rm)) + (fe + fo);
 *           out[q] = (g[q] + (rp - rm)) + (fe - fo);
 * The parenthesised first terms are the lines of the operator without the force.  The split of the source over the two rates is
 * what makes a force-driven Poiseuille profile exact at Lambda = 3/16.  With the subgrid model on, the cell's own om and, with
 * TRT, its own omega_m stand in pe and po where omega and omega_m stand.  The model reads the stress as it does without the
 * force, from the shifted momenta: the -1/2 (uF + Fu) correction of the stress estimate is out of scope.
 *
 * Reported velocity.  The physical velocity of a forced cell is (sum of c_k g[k] + F / 2) / rho on the values g the cell
 * gathers, which is what the shifted momenta are and what av_vels sums.  The library stores the values BEHIND a collision, and
 * the collision above adds the whole force to a cell's momentum: sum of c_k out[k] = sum of c_k g[k] + F.  So on a stored state
 * the physical velocity is (sum of c_k f_k - F / 2) / rho, and with the force on the output stage (lbm_dp_final_state,
 * lbm_dens_final_state and the Reynolds numbers) subtracts 0.5 * F_x and 0.5 * F_y from the two momentum sums of a fluid cell
 * before the division by its density; with it off the statements are untouched.  A state that was uploaded and not yet stepped
 * is read the same way.
 *
 * Nothing else moves: blocked cells bounce back, or go through the statements of "Moving walls", and take no force;
 * accelerate_flow stays and composes (accel = 0 switches it off); the boundary fix, the momentum-exchange force and the body
 * maps, the order of every sum, the Reynolds number's viscosity and both steady criteria are unchanged.  Every bit identity stated
 * for the existing flow holds with the force on: between the kernel forms ("multistep"), launch splits and runs; between a
 * double-precision context and a member of a double-precision ensemble with the same force; between a member stopped by
 * lbm_dsteady_run or lbm_dbody_steady_run at count c and a plain run of c steps.  It composes with "force", body maps, TRT, open
 * boundaries, moving walls and the subgrid model, set in any order.
 *
 * When it is accepted.  Only while steps_done is 0, the rule of lbm_dles_set: otherwise LBM_ERR_STATE.  lbm_dp_upload,
 * lbm_dens_upload and lbm_dp_upload_obstacles keep the setting.  An ensemble has the force on for all members, each with its own
 * pair, or off.  Everything is checked before anything changes: after a refusal nothing has changed, on the host or on the
 * device.
 *
 * Names: lbm_ddrive_*, on both double-precision handles ("body" is the body map, "force" the measured force).  Out of scope: fp32
 * contexts and fp32 ensembles, which get nothing; a force that varies in space or time; a force proportional to the local density.
 */

/* Set the body force of a double-precision context: (0, 0) is off (the default).  LBM_ERR_ARG, before the context is read: a NULL
 * context, a component that is NaN or infinite.  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_ddrive_set(lbm_dp *d, double f_x, double f_y);

/* The force in force ((0, 0): off).  Either output may be NULL; both NULL (f_x_out and f_y_out), or a NULL context: LBM_ERR_ARG. */
int lbm_ddrive_get(const lbm_dp *d, double *f_x_out, double *f_y_out);

/* The same for a double-precision ensemble: f = double[n][2], F_x then F_y of every member, members may differ; NULL: off for all
 * members.  LBM_ERR_ARG, the message names the member: a component that is NaN or infinite, a member whose two components are both
 * zero (its context twin would run the kernels without the force); nothing on the device changes after a refusal.  LBM_ERR_STATE:
 * steps done.  Synchronises. */
int lbm_ddrive_ens_set(lbm_dens *e, const double *f /*[n][2]*/);

/* on_out: 1 while the force is on, else 0; f_out = double[n][2], zeros while it is off.  Either output may be NULL; both NULL
 * (on_out and f_out), or a NULL ensemble: LBM_ERR_ARG. */
int lbm_ddrive_ens_get(const lbm_dens *e, int *on_out, double *f_out /*[n][2]*/);

/*
 * ---- Scalar transport: a passive scalar carried by the flow, for the double-precision families -------------------------------
 *
 * The double-precision families compute a flow; nothing so far is carried by it.  With a scalar on, a context, or each member of
 * an ensemble, carries one field C(x, y) - dye, a concentration, a temperature that does not act back - that the flow advects
 * and that diffuses with a diffusivity D of its own.  The scalar is PASSIVE: the flow never reads it, and the flow with a scalar
 * on equals the flow without it bit for bit (cells, av_vels, the force record).  It is advanced by a kernel of its own
 * (dp_scalar_step); no flow kernel, argument struct or launch changes.  Off by default.  The reference has no counterpart.
 *
 * The lattice.  D2Q5: speeds k = 0..4 are the flow's speeds 0..4 (rest, E, N, W, S), the opposites are 1 <-> 3 and 2 <-> 4, the
 * weights 1/3 (rest) and 1/6.  A handle holds five populations g_k per cell in the row-interleaved layout of the flow (g_k(x, y) at
 * y * 5 * plane_stride + k * plane_stride + x), in two arrays.  The host computes, in double, contraction off,
 *     omega_s = 1.0 / (3.0 * D + 0.5);
 *
 * When a step happens.  Scalar step n runs BEFORE flow step n, on the state that flow step n streams: the current cells after
 * step n's accelerate_flow, whether the run's prologue applied it or the previous launch's fused write did.  So run(10) and
 * run(3); run(7) see the same velocities.  While a scalar is on every launch of a run advances ONE step (the scalar needs each
 * step's velocities); the option "multistep" still chooses the kernel form, and every form computes the same bits.
 *
 * Definition.  A FLUID cell x does the following; all in double, contraction off, one IEEE operation per written operator, in this
 * order.  (u_x, u_y) is the output stage's velocity of the cell's nine stored values (the statements of lbm_dp_final_state; with a
 * body force on, the physical velocity, less half the force).  The gather, with q = x - c_k, periodic in both axes:
 *     h[0] = g[0](x);
 *     for k = 1..4:
 *         q fluid:                           h[k] = g[k](q);
 *         q blocked, c_wall(q) NaN:          h[k] = g[opp(k)](x);
 *         q blocked, c_wall(q) finite:       h[k] = (1.0 / 3.0) * c_wall(q) - g[opp(k)](x);
 * A blocked neighbour with NaN is an insulating wall (half-way bounce-back), one with a finite value a wall held at that value.
 * With open boundaries on ("Open boundaries"), behind the gather:
 *     column 0:         h[1] = c_in(y) - (((h[0] + h[2]) + h[3]) + h[4]);
 *     column nx - 1:    h[3] = g[3](x);
 * the inlet carries the value c_in(y), the outlet the cell's own stored value (zero gradient).  The collision:
 *     C = (((h[0] + h[1]) + h[2]) + h[3]) + h[4];
 *     a_x = 3.0 * (C * u_x);          a_y = 3.0 * (C * u_y);
 *     e[0] = (1.0 / 3.0) * C;
 *     e[1] = (1.0 / 6.0) * (C + a_x);
 *     e[3] = (1.0 / 6.0) * (C - a_x);
 *     e[2] = (1.0 / 6.0) * (C + a_y);
 *     e[4] = (1.0 / 6.0) * (C - a_y);
 *     for k = 0..4:
 *         g'[k] = h[k] + omega_s * (e[k] - h[k]);
 * A BLOCKED cell's five values are copied through unchanged.
 *
 * Reported field.  A fluid cell reports (((g[0] + g[1]) + g[2]) + g[3]) + g[4] of its stored values, a blocked cell 0.0.
 * Setting a scalar initialises g[k] = w_k * c0(x) on every cell: (1.0 / 3.0) * c0 for k = 0, (1.0 / 6.0) * c0 for the others.
 *
 * Bit identities.  A member of a double-precision ensemble equals a double-precision context with the same scalar, flow and
 * obstacles; the kernel forms ("multistep") and launch splits agree; a download followed by an upload changes nothing.
 *
 * When it is accepted.  Between runs at any step count: a scalar is often released into a developed flow.  lbm_dp_upload,
 * lbm_dens_upload and lbm_dp_upload_obstacles keep the scalar and its state; c_wall is only ever read at blocked cells.  An ensemble
 * has the scalar on for all members, each with its own D, c_wall and c_in, or off.  Everything is checked before anything changes:
 * after a refusal nothing has changed, on the host or on the device.  lbm_dsteady_run and lbm_dbody_steady_run are refused
 * (LBM_ERR_ARG) while a scalar is on: a member that stops would need a gated scalar kernel, which is out of scope.
 *
 * Names: lbm_dscalar_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, which get nothing; a
 * scalar that acts back on the flow (buoyancy); more than one scalar per handle; a scalar step fused into the LDS-tile kernels.
 */

/* Set the scalar of a double-precision context: diffusivity > 0 switches it on from the field c0 = double[ny][nx]; c_wall =
 * double[ny][nx] (NaN: insulating, finite: held at that value; read at blocked cells only) or NULL: all insulating; c_in =
 * double[ny], read with open boundaries on, or NULL: zeros.  diffusivity == 0 switches it off: the handle then runs as one that never
 * had a scalar, multi-step launches included.  LBM_ERR_ARG: a NULL context, a negative or non-finite diffusivity, a NULL c0 with a
 * positive diffusivity (these before the context is read), a non-finite c0 or c_in, an infinite c_wall.  Synchronises first. */
int lbm_dscalar_set(lbm_dp *d, double diffusivity, const double *c0 /*[ny][nx]*/, const double *c_wall /*[ny][nx] or NULL*/,
                    const double *c_in /*[ny] or NULL*/);

/* on_out: 1 while the scalar is on, else 0; the diffusivity and omega_s in force, 0.0 while it is off.  Any output may be NULL; all
 * NULL (on_out, diffusivity_out and omega_s_out), or a NULL context: LBM_ERR_ARG. */
int lbm_dscalar_get(const lbm_dp *d, int *on_out, double *diffusivity_out, double *omega_s_out);

/* The reported field, the five populations as double[5][ny][nx], and the populations back.  LBM_ERR_ARG: a NULL argument, or the
 * scalar is off.  Synchronise. */
int lbm_dscalar_field(lbm_dp *d, double *c_out /*[ny][nx]*/);
int lbm_dscalar_download(lbm_dp *d, double *g_out /*[5][ny][nx]*/);
int lbm_dscalar_upload(lbm_dp *d, const double *g /*[5][ny][nx]*/);

/* The same for a double-precision ensemble, every array with a leading member axis: diffusivity = double[n], every entry > 0 and
 * finite, members may differ; NULL: off for all members.  LBM_ERR_ARG, the message names the member: as above, and an entry of
 * diffusivity that is 0.  LBM_ERR_STATE: the ensemble is ragged (lbm_dsteady_run). */
int lbm_dscalar_ens_set(lbm_dens *e, const double *diffusivity /*[n] or NULL*/, const double *c0 /*[n][ny][nx]*/,
                        const double *c_wall /*[n][ny][nx] or NULL*/, const double *c_in /*[n][ny] or NULL*/);
int lbm_dscalar_ens_get(const lbm_dens *e, int *on_out, double *diffusivity_out /*[n]*/, double *omega_s_out /*[n]*/);
int lbm_dscalar_ens_field(lbm_dens *e, double *c_out /*[n][ny][nx]*/);
int lbm_dscalar_ens_download(lbm_dens *e, double *g_out /*[n][5][ny][nx]*/);
int lbm_dscalar_ens_upload(lbm_dens *e, const double *g /*[n][5][ny][nx]*/);

/*
 * ---- Buoyancy: the scalar acts back on the flow, for the double-precision families ------------------------------------------------
 *
 * "Body force" carries one constant force per grid and "Scalar transport" a field the flow never reads; each names the other's
 * missing half as out of scope ("a force proportional to the local density" was the nearest wording there, "a scalar that acts
 * back on the flow (buoyancy)" here).  This section lifts those two remarks: a handle with a scalar on may carry a buoyancy
 * b = (b_x, b_y) and a reference value c_ref, and every fluid cell then takes a force density that follows its own scalar value,
 * the Boussinesq coupling.  That is natural convection in double precision: Rayleigh-Benard layers, heated cavities, plumes, and a
 * sweep over Rayleigh numbers in one ensemble.  Off by default.  The reference has no counterpart.
 *
 * Definition.  All in double, contraction off, one IEEE operation per written operator, in this order.  With g[0..4] the cell's
 * five STORED scalar values (the reported field of "Scalar transport") and F0 = (F0_x, F0_y) the body force of lbm_ddrive_set,
 * (0.0, 0.0) while that is off, every FLUID cell takes the force density
 *     C = (((g[0] + g[1]) + g[2]) + g[3]) + g[4];
 *     d = C - c_ref;
 *     F_x = F0_x + b_x * d;
 *     F_y = F0_y + b_y * d;
 * As with lbm_ddrive_*, the force is NOT multiplied by the cell's density: the acceleration is b d / rho, and a layer of H fluid
 * rows between half-way walls held dC apart has Ra = (|b| dC / rho0) H^3 / (nu kappa).  F stands wherever "Body force" has its
 * constant F: in the half shift of the two momenta, in the source (uF, cF[k], se[k], so[k]), under pe and po; the subgrid rates read
 * the shifted momenta.  Blocked cells take no force.
 *
 * Which scalar state is read.  Everything is a function of the two current states.  Scalar step n still runs before flow step n.
 * Scalar step n forms each cell's F from the scalar array it reads, state n - the force the flow's stored state n already carries -
 * and the velocity it advects with is the output stage's, less half of this F.  Flow step n then forms F from the scalar array
 * that scalar step n has just written, state n + 1.  So after any number of steps the stored flow state carries the force of the
 * scalar state that is current, and the output stage (lbm_dp_final_state, lbm_dens_final_state and the Reynolds numbers) subtracts
 * 0.5 * F_x and 0.5 * F_y of the current scalar state, per cell, from the two momentum sums.  An uploaded state that has not yet
 * been stepped is read the same way, the rule of "Body force".
 *
 * Kernels.  While buoyancy is on the scalar step is dp_scalar_step<true> and the flow step d2q9_dp_buoyant, one step per launch
 * in both families: there is ONE kernel form, and the option "multistep" chooses nothing.  Nothing else moves: accelerate_flow, the
 * boundary fix, moving walls, the subgrid model, TRT, the momentum-exchange force and its record, the order of every sum.  With
 * buoyancy off the passive path runs and keeps every bit.  Bit identities: a member of a double-precision ensemble equals a
 * double-precision context with the same settings; launch splits agree; a download followed by an upload of both states changes
 * nothing; with C == c_ref on every cell for ever (c0 = 0, c_ref = 0, insulating walls) the flow equals the flow under the body
 * force F0 alone, bit for bit.
 *
 * When it is accepted.  Only with a scalar on, and only while steps_done is 0 (the rule of lbm_ddrive_set): otherwise
 * LBM_ERR_STATE.  (0, 0) on a context means off, and is accepted with the scalar off too.  An ensemble has buoyancy on for all
 * members, each with its own triple (b_x, b_y, c_ref), or off (NULL); a member whose b is (0, 0) is refused, the twin rule of
 * lbm_ddrive_ens_set.  Switching the scalar off while buoyancy is on is LBM_ERR_STATE; setting the scalar again, or
 * lbm_dscalar_upload, while buoyancy is on is allowed.  lbm_dp_upload, lbm_dens_upload and lbm_dp_upload_obstacles keep the
 * setting.  Everything is checked before anything changes.  Steady runs stay refused while a scalar is on.
 *
 * Names: lbm_dbuoy_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, which get nothing; the
 * LDS-tile kernels, a fused scalar + flow tile form included; more than one scalar; a density-weighted force; a viscosity that
 * depends on the scalar; switching buoyancy on into a developed flow.
 */

/* Set the buoyancy of a double-precision context: b = (0, 0) is off (the default).  LBM_ERR_ARG, before the context is read: a
 * NULL context, a component or c_ref that is NaN or infinite.  LBM_ERR_STATE: b is not (0, 0) and the scalar is off; steps done.
 * Synchronises. */
int lbm_dbuoy_set(lbm_dp *d, double b_x, double b_y, double c_ref);

/* on_out: 1 while buoyancy is on, else 0; b_out = double[2] and c_ref_out, zeros while it is off.  Any output may be NULL; all NULL
 * (on_out, b_out and c_ref_out), or a NULL context: LBM_ERR_ARG. */
int lbm_dbuoy_get(const lbm_dp *d, int *on_out, double *b_out /*[2]*/, double *c_ref_out);

/* The same for a double-precision ensemble: b = double[n][3], b_x, b_y, c_ref of every member, members may differ; NULL: off for
 * all members.  LBM_ERR_ARG, the message names the member: a value that is NaN or infinite, a member whose b is (0, 0).
 * LBM_ERR_STATE: the scalar is off; steps done.  Synchronises. */
int lbm_dbuoy_ens_set(lbm_dens *e, const double *b /*[n][3] or NULL*/);

/* on_out: 1 while buoyancy is on, else 0; b_out = double[n][3], zeros while it is off.  Either output may be NULL; both NULL (on_out
 * and b_out), or a NULL ensemble: LBM_ERR_ARG. */
int lbm_dbuoy_ens_get(const lbm_dens *e, int *on_out, double *b_out /*[n][3]*/);

/*
 * ---- Scalar record: what the scalar holds and carries per step, and steady runs that stop each member on it -----------------------
 *
 * "Scalar transport" and "Buoyancy" both say that steady runs stay refused while a scalar is on ("a member that stops would need a
 * gated scalar kernel, which is out of scope").  For lbm_dsteady_run and lbm_dbody_steady_run that stands, with the same code and
 * message: their criteria judge the flow alone, and a passive scalar is still moving long after its flow has settled.  This section
 * lifts the remark for a criterion of the scalar's own.  The flow has av_vels and the force record per step; with the record on,
 * the scalar has three sums per step, and lbm_drecord_steady_run stops every member of an ensemble where one of them has settled.
 * Off by default.  The reference has no counterpart.
 *
 * Definition.  Per step t and per member, three sums over the FLUID cells, taken inside scalar step t from values that step holds
 * anyway.  With h[0..4] the cell's five gathered values behind the wall, inlet and outlet statements of "Scalar transport", and
 * (u_x, u_y) the velocity that step advects with (the output stage's; with buoyancy less half of the cell's own force):
 *     c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4];     content: the sum of c
 *     q_x = c * u_x;                                  flux_x:  the sum of q_x
 *     q_y = c * u_y;                                  flux_y:  the sum of q_y
 * c is the collision's own sum and the products are those under its a_x and a_y.  A blocked cell adds +0.0.  All in double,
 * contraction off, one IEEE operation per written operator.
 *
 * Order of summation, fixed as for av_vels: the two cells of a lane (a + b, or a + 0.0 where the lane has no second cell; an idle
 * lane of the row's last segment holds 0.0); the eight lanes of a 16-cell row segment in the tree of xor 1, 2, 4; then the
 * segments of the step, [ny][nseg] per member, through the reduction that av_vels takes (in one stage, or in two where a step has
 * many segments), from a ring of the scalar's own.  A member of an ensemble equals a context, and a run in pieces one run, bit for
 * bit.  flux_x / N_fluid * H / (D dC) is the convective part of the volume-averaged Nusselt number of a side-heated cavity, flux_y
 * the same for a layer heated from below.
 *
 * Nothing else moves.  With the record on the scalar step is dp_scalar_step_rec, the same lane body: cells, scalar populations,
 * av_vels, the force record and the four fields are the same bits with the record on as with it off.
 *
 * When it is accepted.  Only with a scalar on (otherwise LBM_ERR_ARG) and only while steps_done is 0, the rule of lbm_dbuoy_set:
 * LBM_ERR_STATE after a step, until the next upload of the flow.  Switching the scalar off while the record is on is
 * LBM_ERR_STATE.  lbm_dscalar_set with new fields and lbm_dscalar_upload between runs leave the recorded entries as they are; the
 * uploads of the flow keep the setting and start the record anew.
 *
 * Steady runs.  lbm_drecord_steady_run is lbm_dsteady_run in everything but the criterion: the legs, check points, polling, limits
 * and the words of lbm_dsteady_steps are those of "Steady runs of a double-precision ensemble".  A(s) is entry s - 1 of the chosen
 * value's record of the member as lbm_drecord_ens returns it, nothing multiplied into it; a member stops at a check point s
 * where fabs(A(s) - A(s - window)) <= rel_tol * fabs(A(s)), difference and bound as separate statements.  A leg launches, per step
 * and under the members' words: the scalar step dp_scalar_step_rec, and the flow step d2q9_dp_ensemble_gated at depth 1 or, with
 * buoyancy, d2q9_dp_buoyant_gated.  A member stopped at count c holds the bits of an lbm_dens_run(e, c) in one piece, cells, scalar
 * and every record.  Afterwards a ragged ensemble is read member by member from the array that holds each (lbm_dscalar_ens_field,
 * lbm_dscalar_ens_download, the fields with buoyancy); lbm_dscalar_ens_set and lbm_dscalar_ens_upload are refused with
 * LBM_ERR_STATE until lbm_dens_upload, which keeps every member's scalar state, unchanged.
 *
 * Names: lbm_drecord_*, on both double-precision handles, beside lbm_dscalar_* (the ten entry points of "Scalar transport").  Out
 * of scope: fp32 contexts and fp32 ensembles, which get nothing; a criterion on more than one value; wall fluxes (the conductive
 * part of a Nusselt number is a difference of the reported field).
 */

/* Switch the record of a double-precision context on (1) or off (0, the default).  LBM_ERR_ARG: a NULL context, a value other than
 * 0 and 1, the scalar is off.  LBM_ERR_STATE: steps done.  Synchronises. */
int lbm_drecord_set(lbm_dp *d, int on);

/* on_out: 1 while the record is on, else 0.  A NULL argument: LBM_ERR_ARG. */
int lbm_drecord_get(const lbm_dp *d, int *on_out);

/* The three records, lbm_dp_steps_done(d) entries each.  Any output may be NULL; all three NULL, or a NULL context: LBM_ERR_ARG,
 * before a device is touched.  LBM_ERR_STATE: the record is off.  Synchronises. */
int lbm_drecord(lbm_dp *d, double *content_out /*[steps_done]*/, double *flux_x_out /*[steps_done]*/,
                       double *flux_y_out /*[steps_done]*/);

/* The same for a double-precision ensemble, all members on or off together: double[n][steps_done] per value; a member that
 * lbm_drecord_steady_run stopped earlier holds +0.0 from its own count on (lbm_dforce_ens_record's rule). */
int lbm_drecord_ens_set(lbm_dens *e, int on);
int lbm_drecord_ens_get(const lbm_dens *e, int *on_out);
int lbm_drecord_ens(lbm_dens *e, double *content_out /*[n][steps_done]*/, double *flux_x_out /*[n][steps_done]*/,
                           double *flux_y_out /*[n][steps_done]*/);

/* Advance every member until ITS OWN record of the scalar has settled, at most max_steps steps (beside lbm_dsteady_run, whose
 * refusals it shares).  which: 0 content, 1 flux_x, 2 flux_y.  LBM_ERR_ARG, before a device is touched: a NULL ensemble, max_steps
 * < 0, window < 1, rel_tol negative or not finite, which outside 0 .. 2, the record is off.  Synchronises. */
int lbm_drecord_steady_run(lbm_dens *e, int max_steps, int window, double rel_tol, int which);

/*
 * ---- Running statistics: time means and Reynolds stresses, sums over time per cell ------------------------------------------------
 *
 * The records above (av_vels, the force, the scalar) are sums over space per step.  This section adds the other half, sums over
 * time per cell: with statistics on, a context holds six sums per cell, double[6][ny][nx], and a sample count; each member of an
 * ensemble holds its own.  Off by default.  The reference has no counterpart.
 *
 * Definition.  A sample at step count s reads the four fields exactly as lbm_dp_final_state (lbm_dens_final_state) would return
 * them after s steps: the half-force corrections of "Body force" and "Buoyancy" included, and a blocked cell giving 0, 0, 0,
 * density / 3.  Per cell, all in double, contraction off, one IEEE operation per written operator:
 *     S[0] = S[0] + u_x;
 *     S[1] = S[1] + u_y;
 *     S[2] = S[2] + pressure;
 *     S[3] = S[3] + u_x * u_x;
 *     S[4] = S[4] + u_y * u_y;
 *     S[5] = S[5] + u_x * u_y;
 * Samples are taken in order of s, so every S[v] is a left-to-right sum; there is no cross-lane or cross-cell arithmetic, so no
 * order of summation needs fixing.  The means are S[0..2] / samples, the Reynolds stresses S[3] / samples - mean(u_x)^2 and so on,
 * formed by the caller.  Raw sums have a caveat: a covariance loses as many digits as the variance is small against the squared
 * mean (fluctuations of 1e-3 on a mean of 0.1 keep about 10 digits in double).
 *
 * When a sample is taken.  lbm_dstats_set(d, every) with every >= 1 switches the statistics on: it allocates the six planes (48 B
 * per cell beside the 144 B of the two grids), sets them to +0.0, sets the sample count to 0 and the origin s0 to the step count
 * as it stands.  It is accepted between runs at ANY step count: statistics usually start behind a transient.  Samples are taken at
 * every step count s = s0 + j * every, j >= 1, that a run reaches: a run of nsteps from step count `first` takes the sample points
 * in (first, first + nsteps].  A run in pieces takes the samples of one run and leaves the same bits.  Setting again while on
 * starts anew, with zeros and a new origin; every may change.  every == 0 switches the statistics off and frees the planes.
 * lbm_dp_upload, lbm_dens_upload and lbm_dp_upload_obstacles keep the setting and start the statistics anew, the origin at the
 * step count behind the upload.
 *
 * How a run takes them.  The run is cut at its sample points.  Every piece is enqueued the way a run of its length is: the
 * prologue accelerate_flow (none with open boundaries), launches of equal depth within the piece (one step each with a scalar
 * on), the next step's acceleration fused only inside the piece.  Behind a piece that ends on a sample point one kernel,
 * dp_stats_sample, reads the current arrays - the state the output stage would read - and adds to the planes.  The ring of
 * per-step segment sums and its flushes carry across the cuts: a cut costs one sample launch and one accelerate launch, no
 * synchronisation and no reduction launch.
 *
 * Nothing else moves.  lbm_dp_run(a) then lbm_dp_run(b) equals lbm_dp_run(a + b) bit for bit, in both families and with every
 * option; a run with statistics on is such a run in pieces with a kernel between them that writes the planes alone.  So cells,
 * av_vels, the force record, the fields, the Reynolds number, the scalar and its record are the same bits with statistics on as
 * with them off.
 *
 * When it is refused.  Everything is checked before anything changes.  LBM_ERR_ARG: a NULL handle, every < 0, all-NULL outputs of
 * a getter.  LBM_ERR_ARG, as long as statistics are on, from lbm_dsteady_run, lbm_dbody_steady_run and lbm_drecord_steady_run,
 * with a message that names lbm_dstats_ens_set: a member that stops would need a gated sample kernel, which is out of scope.
 * LBM_ERR_STATE: lbm_dstats_ens_set with every >= 1 on a ragged ensemble; lbm_dstats / lbm_dstats_ens while the statistics are
 * off.  LBM_ERR_HIP: the planes do not fit the device's memory; statistics are then off and nothing else has changed.
 *
 * Names: lbm_dstats_*, on both double-precision handles.  Out of scope: fp32 contexts and fp32 ensembles, which get nothing;
 * moments of the scalar (the mean of C, turbulent heat fluxes); steady runs with statistics on; a per-member every; statistics
 * fused into a flow kernel; shifted or Welford accumulation.
 */

/* Switch the statistics of a double-precision context on (every >= 1: a sample every so many steps from now) or off (0, the
 * default).  LBM_ERR_ARG, before the context is read: a NULL context, every < 0.  LBM_ERR_HIP: no memory for the planes.
 * Synchronises. */
int lbm_dstats_set(lbm_dp *d, int every);

/* every_out: the setting, 0 while off; origin_out: the step count the sample points are counted from; samples_out: the samples
 * taken since.  Zeros while off.  Any output may be NULL; all three NULL, or a NULL context: LBM_ERR_ARG. */
int lbm_dstats_get(const lbm_dp *d, int *every_out, int *origin_out, int *samples_out);

/* The six planes of sums.  LBM_ERR_ARG: a NULL argument.  LBM_ERR_STATE: the statistics are off.  Synchronises. */
int lbm_dstats(lbm_dp *d, double *sums_out /*[6][ny][nx]*/);

/* The same for a double-precision ensemble: one every for all members, each member its own planes, all with one origin and one
 * count.  LBM_ERR_STATE: every >= 1 on a ragged ensemble. */
int lbm_dstats_ens_set(lbm_dens *e, int every);
int lbm_dstats_ens_get(const lbm_dens *e, int *every_out, int *origin_out, int *samples_out);
int lbm_dstats_ens(lbm_dens *e, double *sums_out /*[n][6][ny][nx]*/);

const char *lbm_last_error(void);
const char *lbm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LBM_H */
