/* zkhip.h — C ABI of libzkhip.so, the MI355X-native Groth16 proving backend.
 *
 * This is the drop-in boundary for ONE reference path: `Backend<T, G16>::generate_proof`
 *   trait      /root/reference/zokrates_proof_systems/src/lib.rs:98-112
 *   CPU impl   /root/reference/zokrates_ark/src/groth16.rs:20-53   (`impl Backend<T,G16> for Ark`)
 *   call site  /root/reference/zokrates_cli/src/ops/generate_proof.rs:187
 * A Rust crate `zokrates_hip` (source in INTEGRATION.md) implements that trait by calling the
 * functions below; everything above the trait (CLI, JSON, Solidity export, verify) is untouched.
 *
 * Conventions
 *  - Every function returns int32_t: 0 = ZKHIP_OK, < 0 = error class; text via zkhip_last_error().
 *    The library never throws across the boundary and never aborts.  (The reference panics on any
 *    failure — zokrates_ark/src/groth16.rs:41-44 `.unwrap()` — so the Rust shim turns non-zero
 *    into `panic!`.)
 *  - Field elements cross the boundary as canonical little-endian bytes (32 B for Fr; sz(Fq) =
 *    32 B for bn128, 48 B for bls12_381 and bls12_377): the bytes of ark `ToBytes` / `Field::write`
 *    (/root/reference/zokrates_field/src/lib.rs:215-226).  Neither side needs the other's
 *    Montgomery constant.
 *  - Caller owns every input buffer for the duration of the call; the library copies what it
 *    keeps; outputs go to caller-allocated buffers; long-lived objects are opaque handles with
 *    paired create/free.  No callbacks.
 *  - A context is bound to one GPU and is not re-entrant (one call at a time per context);
 *    distinct contexts may be used from distinct threads.
 *  - One pair of calls leaves a proof in flight ACROSS calls: zkhip_prove_g16_split_begin .. zkhip_prove_g16_split_end.  Between
 *    them the proof is PENDING in its context, and the context accepts zkhip_prove_g16_split_end, zkhip_prove_g16_split_abort and
 *    the calls that neither enqueue device work nor change a handle (zkhip_last_error, zkhip_describe, zkhip_pk_dims,
 *    zkhip_pk_is_bound, zkhip_pk_export_size, zkhip_partial_size, zkhip_combine_*, zkhip_ctx_set_checked(ctx, -1),
 *    zkhip_ctx_unsatisfied, zkhip_setup_*_size, the zkhip_prog_* family, zkhip_xplan_levels, zkhip_exec_last).  Every other call on that context or on one of its keys —
 *    the prove calls, zkhip_r1cs_check, a second begin, zkhip_pk_bind_r1cs / _shard / zkhip_pk_unbind, zkhip_ctx_tune,
 *    zkhip_ctx_set_checked(ctx, 0 / 1), key loads, imports and exports, setups, uploads (zkhip_assignment_upload, _upload_packed,
 *    _upload_witness), zkhip_wplan_create (it enqueues the copies of its tables) and the primitives (they work in the
 *    pending proof's buffers and on its streams) — returns ZKHIP_ERR_BAD_ARG with a message that names the pending split proof,
 *    before anything is enqueued, and leaves the pending proof as it is.  Freeing a handle a pending proof uses is the caller's
 *    error, as it is during any call.
 *  - A proof queue (zkhip_queue_open .. zkhip_queue_close, below) keeps up to its capacity of proofs in flight across calls — the
 *    pipeline of the *_batch calls with the caller as the loop.  Order and capacity: capacity is the context's ZKHIP_TUNE_SLOTS when
 *    the queue is opened; tickets count from 0 per queue; collect is first in, first out; a submit at capacity returns ZKHIP_ERR_BUSY and
 *    a collect on an empty queue ZKHIP_ERR_BAD_ARG, and neither changes anything; proofs are enqueued exactly as the batch calls enqueue
 *    theirs, slots round-robin, so submit, submit, submit, collect, submit, collect ... is the batch calls' own schedule.  Bytes: every
 *    collected proof is byte-identical to what zkhip_prove_g16 / zkhip_prove_gm17 returns for the same inputs, for any order of calls,
 *    a bound or an unbound key, and each of the four witness sources (host z, resident, packed, witness file).  Buffers: z, packed, the
 *    bytes of a witness file and rnd belong to the caller again as soon as
 *    submit returns (the library copies host memory through its own pinned ring; the measurement switch ZKHIP_COPY_MODE=0, which
 *    hands the caller's pointer to the runtime instead, gives that up); a resident assignment must stay alive until its ticket is
 *    collected.  Failures of ONE proof fail that ticket only
 *    and leave every other proof in flight as it is: an entry that is not canonical (found on the device; ZKHIP_ERR_BAD_ARG at collect,
 *    the message of zkhip_prove_g16), an assignment that does not satisfy the system in checked mode (ZKHIP_ERR_UNSATISFIED at collect,
 *    the output zero-filled, the message names the ticket and the constraint, zkhip_ctx_unsatisfied reports one triple with proof index
 *    0), and a submit refused for its arguments — null or both sources, z[0] != 1, a blinding scalar that is not canonical, an assignment
 *    of another system, a malformed packed buffer (ZKHIP_ERR_PARSE, the messages of zkhip_assignment_upload_packed), a witness file whose
 *    length does not match its count or a plan of another system (zkhip_queue_submit_witness) — which consumes no
 *    ticket.  A witness file's own defects, found on the device — a value that is not canonical, an id out of range (ZKHIP_ERR_PARSE), a
 *    variable without a value (ZKHIP_ERR_UNSATISFIED) — fail their ticket at collect like the others, with the host reader's messages.  Only a device error breaks the queue: it is kept, every ticket still in flight collects with ZKHIP_ERR_DEVICE and its text,
 *    further submits answer the same, and zkhip_queue_close still works.  Pending: an open queue makes its context pending in the sense
 *    of the split-proof paragraph above — every call that paragraph refuses is refused, on the host and before anything is enqueued,
 *    with ZKHIP_ERR_BAD_ARG and a message that names the open queue (zkhip_prove_g16_split_begin and a second zkhip_queue_open among
 *    them; zkhip_queue_open while a split proof is pending gets that paragraph's message); the calls it lets through stay allowed
 *    (zkhip_prove_g16_split_end finds nothing pending, zkhip_prove_g16_split_abort has nothing to drop).  Checked mode is read when the
 *    queue is opened.  Freeing the key, the constraint system or the context under an open queue is the caller's error.  Resources:
 *    opening, submitting and collecting create no stream and no event beyond the ones the proof slots own, and allocate nothing once
 *    every slot has been used (a packed buffer longer than any before grows the context's one buffer for packed bytes, a witness file
 *    longer than any before the context's one buffer for file bytes): a process near
 *    the hardware-queue budget of INTEGRATION.md section 4 stays where it is.
 *  - There is no CPU fallback: without a usable gfx950 device zkhip_ctx_create fails with
 *    ZKHIP_ERR_DEVICE.
 */
#ifndef ZKHIP_H
#define ZKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKHIP_OK 0
#define ZKHIP_ERR_BAD_ARG (-1)      /* null pointer, size mismatch, unsupported curve/size        */
#define ZKHIP_ERR_PARSE (-2)        /* malformed proving key / non-canonical field element         */
#define ZKHIP_ERR_NOMEM (-3)        /* host or device allocation failed                            */
#define ZKHIP_ERR_DEVICE (-4)       /* no GPU, HIP runtime error, kernel launch failure            */
#define ZKHIP_ERR_UNSATISFIED (-5)  /* the assignment does not satisfy the R1CS: zkhip_r1cs_check, and the single-GPU prove calls of a
                                     * context in checked mode (zkhip_ctx_set_checked); also zkhip_prog_assignment and the device
                                     * route of a witness file (zkhip_assignment_upload_witness, a ticket of
                                     * zkhip_queue_submit_witness) for a variable the witness file gives no value                   */
#define ZKHIP_ERR_BUSY (-6)         /* zkhip_queue_submit*: as many proofs in flight as the queue holds; collect one first        */

/* curve ids; names are zokrates_common::constants (/root/reference/zokrates_common/src/constants.rs:5-9) */
#define ZKHIP_CURVE_BN128 0
#define ZKHIP_CURVE_BLS12_381 1
#define ZKHIP_CURVE_BLS12_377 2

typedef struct zkhip_ctx zkhip_ctx;
typedef struct zkhip_pk zkhip_pk;
typedef struct zkhip_r1cs zkhip_r1cs;
typedef struct zkhip_assignment zkhip_assignment;
typedef struct zkhip_vk zkhip_vk;             /* a verifying key resident on the GPU (zkhip_vk_load_g16 / _gm17) */
typedef struct zkhip_prog zkhip_prog;         /* a parsed ZoKrates program (the zkhip_prog_* family below) */

/* Per-proof phase timings in milliseconds (HIP events on the library's own streams).  The MSMs run on their own
 * streams concurrently with each other and with the NTT pipeline, so the phase intervals overlap: they do not
 * add up to total_ms.
 * Replaces nothing in the reference (it has no prover timers) — added observability. */
typedef struct zkhip_timings {
    float h2d_ms;       /* assignment upload + Montgomery conversion                */
    float matvec_ms;    /* K1: sparse A,B,C mat-vec                                  */
    float ntt_ms;       /* K2-K4: 7 transforms + pointwise quotient                  */
    float msm_h_ms;     /* K5: h_query MSM (scalar prep + buckets + reduce)          */
    float msm_z_ms;     /* K6-K8: a/b_g1/l (G1) and b_g2 (G2) MSMs over z            */
    float finish_ms;    /* K9: window combine, assembly, to-affine (host)            */
    float total_ms;     /* wall clock of the whole call                              */
    float kernel_msm_accum_g1_ms; /* sum of G1 bucket-accumulation kernel time       */
    float kernel_msm_accum_g2_ms; /* G2 bucket-accumulation kernel time              */
    float kernel_ntt_ms;          /* the transform passes + quotient kernel, first launch to last (events) */
    float reserved[6];
} zkhip_timings;

/* ---- process-wide start options ---- */
/* The library keeps ~20 HIP streams busy per context (a stream per proof slot and MSM, the transform pipeline, staging, copy-out);
 * the HIP runtime multiplexes them onto GPU_MAX_HW_QUEUES hardware queues (default 4), and kernels of streams that share a queue
 * serialise: 8 queues measured +4 % proofs/s over 4, 16 another +1.5-2 %.  The runtime reads that setting ONCE, when it
 * initialises (the first HIP call of the process) — so it is the HOST's decision, made explicitly here and nowhere else: the
 * library itself never touches the process environment (rounds 1-5 did, in a load-time constructor: a drop-in loaded into someone
 * else's process must not change HIP's behaviour for code that is not its own).
 *   hw_queues > 0: ask the runtime for that many queues — GPU_MAX_HW_QUEUES is set unless the process has set it already;
 *                  effective only BEFORE the first HIP call of the process (ZKHIP_ERR_BAD_ARG once this library has made one).
 *                  8 is safe for any process; 16 only for a process with ONE resident prover (every queue reserves scratch
 *                  for the largest kernel frame launched on it: a process with many contexts ran out at 16).
 *   hw_queues = 0: nothing is changed; the call only reports (returns ZKHIP_OK).
 * Not calling zkhip_init at all is legal: the runtime's own default applies.  Not thread-safe against concurrent getenv in other
 * threads (setenv never is): call it from the thread that starts the process's GPU work, before the others exist. */
int32_t zkhip_init(int32_t hw_queues);

/* ---- context ---- */
/* Number of usable HIP devices (0 if none / no runtime). */
int32_t zkhip_device_count(void);
/* PCI address of HIP device `device` as "dddd:bb:dd.f" (NUL-terminated, at most cap bytes): what ties a device ordinal to the
 * host's view of the same GPU — /sys/bus/pci/devices/<address>/numa_node for the NUMA node a rank's host thread should run
 * on, .../hwmon for clocks and power under load.  No context needed. */
int32_t zkhip_device_pci_bus_id(int32_t device, char* out, size_t cap);
/* Create a context on HIP device `device`. */
int32_t zkhip_ctx_create(int32_t device, zkhip_ctx** out);
void zkhip_ctx_free(zkhip_ctx* ctx);
/* Last error text of this context (or of the failed create when ctx == NULL). Never NULL. */
const char* zkhip_last_error(const zkhip_ctx* ctx);
/* Measurement aid: the shader clock the device actually runs at over the next `duration_us` microseconds, in GHz — ONE wavefront
 * (a few registers, asleep between its two readings) compares the shader-cycle counter with the constant-rate wall clock, on a
 * stream of its own, so that it can run BESIDE whatever else the device is doing: called from a second host thread on a second
 * context of the same device while the first proves, it reads the clock the proving kernels run at (bench.py prices the
 * accumulation's VALU issue limit with it instead of a clock derived from counters).  Blocks for the duration. */
int32_t zkhip_ctx_clock_probe(zkhip_ctx* ctx, uint32_t duration_us, double* ghz_out);

/* Development / measurement knobs of one context (none changes a result; all are plain fields read by the host code,
 * nothing consults the environment after zkhip_ctx_create).  ZKHIP_TUNE_MSM_C: window width of the MSM tables built by
 * later key loads and of later ad-hoc MSMs (0 = automatic); _MSM_WAVES: accumulation waves per SIMD (0 = per point
 * type); _MSM_LANES: number of slices the sorted list is cut into (0 = one per resident work-item); _MSM_MIN_SLICE: the
 * finest cut; _FOLD_SCAN: 0 selects the double-and-add form of the last fold step; _SERIAL: 1 puts every kernel on one
 * stream (un-overlapped per-kernel timing); _NTT_SINGLE_MAX_LOG: largest domain transformed in a single pass;
 * _NTT_COLS: adjacent columns per workgroup of the NTT cols pass; _SLOTS: proofs in flight in the batch calls (1..4);
 * _Z_GATE: which accumulations over the assignment wait for the witness map of their proof (0 none, 1 the three G1
 * lanes — the default —, 2 the G2 lane as well); _FUSE_Z: 0 runs the three G1 MSMs over the assignment as separate
 * launches instead of one; _MSM_FUSED_WAVES: accumulation waves per SIMD of that one launch (0 = per point type);
 * _STREAM_JITTER: race-hunting mode, process-wide — before every kernel launch, copy and fill the library enqueues, a
 * spin kernel of random length (0 .. value microseconds, value <= 5000; 0 = off) is put on the same stream with
 * probability 1/2, so that the relative timing of the library's streams differs from call to call; an ordering that is
 * not carried by an event then shows up as a wrong result instead of passing by luck (tests/test_stream_jitter.py). */
#define ZKHIP_TUNE_MSM_C 1
#define ZKHIP_TUNE_MSM_WAVES 2
#define ZKHIP_TUNE_MSM_LANES 3
#define ZKHIP_TUNE_MSM_MIN_SLICE 4
#define ZKHIP_TUNE_FOLD_SCAN 5
#define ZKHIP_TUNE_SERIAL 6
#define ZKHIP_TUNE_NTT_SINGLE_MAX_LOG 7
#define ZKHIP_TUNE_NTT_COLS 8
#define ZKHIP_TUNE_SLOTS 9
#define ZKHIP_TUNE_Z_GATE 10
#define ZKHIP_TUNE_FUSE_Z 11
#define ZKHIP_TUNE_MSM_FUSED_WAVES 12
#define ZKHIP_TUNE_STREAM_JITTER 13
/* (14, 15: the knobs of the wide-window sort and fold round 3 built and round 4 removed) */
#define ZKHIP_TUNE_MSM_SETS 17        /* bucket sets of the MSM tables built by later key loads: 1 = every window multiple of every base
                                      * (one bucket set per MSM), 2 = every second multiple (two sets) ...; 0 = automatic: 1 while the
                                      * tables fit the device, else the smallest power of two that does (keys above 2^24 constraints) */
#define ZKHIP_TUNE_SKIP_INF 18        /* how the bucket accumulation meets bases at infinity: 0 = per table, from a count made at key load
                                      * (a table with more than one such base in 2048 lets lanes sit them out, the others send the rare
                                      * one through the general code), 1 = lanes always sit them out, 2 = always the general code        */
#define ZKHIP_TUNE_B_SORT 19          /* keys loaded from now on: the MSMs over b_query (G2, and G1 of a Groth16 key) on a sorted list of
                                      * their own that leaves out the variables whose B bases are the point at infinity — 0 = when a tenth
                                      * of them are (real circuits: every variable that does not occur in B), 1 = always, 2 = never       */
/* (21-24, 27: a lone proof's layouts, the transforms' start skew, the sort's placement selector, the one-launch fold, fold chains on second streams:
 * measured, left off and removed — DESIGN.md section 3 names the evidence.  Retired numbers are not reused) */
#define ZKHIP_TUNE_PIPE_PLAN 28        /* 1: every stream of the context made at its first proof and placed on the chip's four dispatchers by plan (core.cuh
                                         make_pipe_streams, ZK_PIPE_PLAN_RESIDENT: a layout found by a local search over four workloads, tools/plan_search.py;
                                         16 streams: ask zkhip_init for 16 queues).  For long-lived provers: level or better than streams in order of first use on
                                         every measured workload (stdlib SHA-256 +8-9 % proofs/s, a lone dense 2^20 proof 0.3 ms sooner); a one-proof process
                                         pays 0.15 s for the streams.  0 (default): streams made as they are first used.  Chosen before the first proof */
#define ZKHIP_TUNE_NTT_FUSE_FIRST 26   /* 1 (default): the first butterfly round of a transform pass on the elements as they are fetched; 0: through LDS like the others */
#define ZKHIP_TUNE_FOLD_HG 25          /* shares a column of the bucket matrix is cut into by the fold's column pass (a power of two <= 256) */
#define ZKHIP_TUNE_HEAVY_RUNS 20      /* 1 (default): the partials of a bucket spread over many slices (the ones of a witness of bits) are
                                      * first summed run by run by a kernel of their own; 0: by the one workgroup of the bucket's row      */
#define ZKHIP_TUNE_NTT_MAX_SUBLOG 16 /* log2 of the longest sub-transform of an NTT pass (2..11; default 11): domains above 2^(2 x this)
                                      * take three passes instead of two — a test hook to reach the three-pass path (domains above
                                      * 2^22) with small domains.  Keys loaded before a change must be reloaded (their h order)        */
#define ZKHIP_TUNE_EXEC_CHUNK 29       /* instances per chunk of zkhip_compute_witness (1 .. 65535 x 64); 0 (default): as many whole waves as fit half of the
                                         device memory that is free (or held by the context's buffers of an earlier call), 32 GiB and 65536 instances at most, at
                                         the bytes a chunk keeps per instance: (zkhip_xplan_dims [7]) of value store, the arguments, and the file and the inputs
                                         where they are asked for.  A test hook as well: it puts the chunk seams wherever a tiny program needs them */
#define ZKHIP_TUNE_EXEC_WIDE 31        /* 0 (default): zkhip_compute_witness runs one work-item per instance, as before.  1: it takes the level-scheduled route —
                                         one work-item per (instruction of a level, instance): the route for a lone instance or a few.  Read at each call;
                                         changes no result */
#define ZKHIP_TUNE_EXEC_WIDE_MIN 32    /* the width (instructions) at and above which a level of the schedule gets a launch of its own on the level-scheduled
                                         route; narrower neighbours share one launch of one workgroup per instance.  0 = the default (1024: the measured sweep was flat); otherwise
                                         1 .. 2^20.  A test hook as well, like _EXEC_CHUNK: it puts the segment seams where a tiny program needs them */
#define ZKHIP_TUNE_ALLOC_FILL 30       /* TESTS ONLY, process-wide (every context of the process, like _STREAM_JITTER), never read from the environment.  A 32-bit
                                         word; while it is non-zero every device and pinned-host block the library allocates is filled with it, to its last byte,
                                         before the allocation returns (one fill and one synchronisation per allocation).  0 (default): off, allocations are
                                         handed out as the runtime gives them.  Fresh memory that reads as zero looks like points at infinity, zero scalars and
                                         empty buckets; under a fill a kernel that reads a slot nobody wrote gives other bytes (tests/test_workspace_reuse.py).
                                         Blocks allocated before the call keep what they hold */
int32_t zkhip_ctx_tune(zkhip_ctx* ctx, int32_t which, int32_t value);

/* ---- proving key ----
 * Replaces `ProvingKey::<E>::deserialize_unchecked(proving_key)` at
 * /root/reference/zokrates_ark/src/groth16.rs:40-42: `bytes` is exactly the `proving.key` file the
 * reference's `setup` writes (zokrates_ark/src/groth16.rs:97-98, ark `serialize_unchecked`:
 * vk{alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1[]}, beta_g1, delta_g1, a_query[],
 * b_g1_query[], b_g2_query[], h_query[], l_query[]; Vec = u64 LE length + elements; affine points
 * uncompressed, infinity = bit 6 of the last byte).  Points are uploaded, converted to Montgomery
 * form and laid out for the MSM kernels; like the reference ("unchecked") no on-curve or subgroup
 * check is made. */
int32_t zkhip_pk_load_g16(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_pk** out);
void zkhip_pk_free(zkhip_pk* pk);
/* Shape of a loaded key: out[0]=m (a_query len), out[1]=N-1 (h_query len), out[2]=w (l_query len),
 * out[3]=l (gamma_abc len). */
int32_t zkhip_pk_dims(const zkhip_pk* pk, uint64_t out[4]);

/* ---- constraint system ----
 * Replaces the `ConstraintSystem` that `Computation::generate_constraints`
 * (/root/reference/zokrates_ark/src/lib.rs:80-129) builds on every call: the three R1CS matrices in
 * CSR form, columns in ark variable order (column 0 = ONE, columns < l instance, then witness).
 * n = constraints, l = num_instance, w = num_witness.  val* = nnz x 32 B canonical LE. */
int32_t zkhip_r1cs_load(zkhip_ctx* ctx, int32_t curve, uint64_t n, uint64_t l, uint64_t w,
                        const uint64_t* rowptr_a, const uint32_t* col_a, const uint8_t* val_a,
                        const uint64_t* rowptr_b, const uint32_t* col_b, const uint8_t* val_b,
                        const uint64_t* rowptr_c, const uint32_t* col_c, const uint8_t* val_c,
                        zkhip_r1cs** out);
void zkhip_r1cs_free(zkhip_r1cs* r1cs);

/* ---- the hot path ----
 * Replaces `Groth16::<E>::prove(&pk, computation, rng)` at /root/reference/zokrates_ark/src/groth16.rs:44
 * ([UPSTREAM] ark_groth16::create_random_proof).
 *   z        : m x 32 B, full assignment in ark order (z[0] must be 1)
 *   r, s     : the two blinding scalars (32 B each).  They are inputs so that the Rust shim samples
 *              them from the caller's RNG exactly as ark does (`Fr::rand(rng)` twice, r then s).
 *   proof_out: 8 x sz(Fq) bytes  A.x A.y | B.x.c0 B.x.c1 B.y.c0 B.y.c1 | C.x C.y  (canonical LE),
 *              then 3 bytes: infinity flags of A, B, C  — the same bytes ark `ToBytes` gives
 *              `parse_g1`/`parse_g2` (/root/reference/zokrates_ark/src/lib.rs:150-218).
 *   timings  : optional. */
int32_t zkhip_prove_g16(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z,
                        const uint8_t* r, const uint8_t* s, uint8_t* proof_out, zkhip_timings* timings);

/* The same with the assignment already resident in HBM (a prover service uploads the witness of proof
 * k+1 while proof k runs; bench.py times this entry point so that the timed region starts with every
 * input in device memory).  zkhip_assignment_upload checks z[0] == 1 and copies m x 32 B to the GPU. */
int32_t zkhip_assignment_upload(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment** out);
void zkhip_assignment_free(zkhip_assignment* z);
int32_t zkhip_prove_g16_resident(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_assignment* z,
                                 const uint8_t* r, const uint8_t* s, uint8_t* proof_out, zkhip_timings* timings);

/* ---- compact assignments ----
 * An assignment of a program over bool / u8 / u32 / u64 is mostly zeros and ones (bit decompositions), and m x 32 B of it cross the
 * bus for every proof.  The packed form keeps the low bytes a value needs and is widened on the device: the upload below returns the
 * same resident assignment as zkhip_assignment_upload, bit for bit, so every *_resident entry point gives the same proof bytes.
 * All integers little-endian; every section starts on a 16-byte boundary of the buffer:
 *
 *   0    8 B   magic "ZKHIPZ1\0"
 *   8    u64   m                      number of elements
 *   16   u64   payload_bytes          multiple of 16
 *   24   u32   block = 1024           elements per block (the only value accepted)
 *   28   u32   flags = 0
 *   32   tags     2 bits per element: element i in bits 2(i%4)..2(i%4)+1 of byte i/4; ceil(m/4) bytes, zero-padded to a
 *                 multiple of 16
 *   ..   index    nblocks + 1 entries of u64, nblocks = ceil(m/1024): index[b] = offset of block b's values inside the payload,
 *                 index[0] = 0, index[nblocks] = payload_bytes, every entry a multiple of 16; one zero entry appended if needed
 *                 to make the count even
 *   ..   payload  per block, in element order: the value's low bytes, width by tag - 0: none (value 0), 1: 1 byte, 2: 8 bytes,
 *                 3: 32 bytes; zero bytes up to the next multiple of 16 at the end of every block (a block: at most 32 KiB)
 *
 * zkhip_assignment_pack is deterministic and minimal (the smallest class that holds the value, all padding zero): two packings of
 * one assignment are the same bytes.  The decoders accept a wider class than needed and decode it to the same value.  A dense
 * witness (field elements: Poseidon) packs to *len >= 32 m, and its caller keeps the plain upload.
 *
 * The packer has no curve: it refuses a z entry that is canonical in NO supported field (>= the largest r, BLS12-381's), and a
 * `cap` that is too small (*len is the length needed either way; nothing is written past cap).  Whether a 32-byte value is below
 * the r of the constraint system's curve is tested where the curve is known: by zkhip_prog_assignment_packed on the host, and by
 * zkhip_assignment_upload_packed on the device, with the error zkhip_assignment_upload gives.
 *
 * zkhip_assignment_unpack and zkhip_assignment_upload_packed validate the whole structure on the host before anything else
 * happens (ZKHIP_ERR_PARSE, the message names the rule): magic, block, flags; len == header + tags + index + payload; the index
 * monotone and 16-aligned; every index span the 16-rounded sum of its block's widths; unused tag bits and padding zero.  The upload
 * then wants m == l + w of `r1cs` and element 0 == 1 (ZKHIP_ERR_BAD_ARG), and is refused like every upload while a split proof is
 * pending.  The context keeps one device buffer for the packed bytes, as large as the largest packed buffer it has uploaded
 * (about 32 m bytes after a dense one), until zkhip_ctx_free.
 * zkhip_assignment_pack is therefore NOT a test that z is canonical for a given curve: only the upload and
 * zkhip_prog_assignment_packed are. */
/* host only: no context, no device work (like the zkhip_prog_* family) */
int32_t zkhip_assignment_pack_bound(uint64_t m, uint64_t* bytes);                 /* worst case: every element 32 bytes wide */
int32_t zkhip_assignment_pack(const uint8_t* z, uint64_t m, uint8_t* out, uint64_t cap, uint64_t* len);
int32_t zkhip_assignment_unpack(const uint8_t* packed, size_t len, uint8_t* z_out, uint64_t m_cap, uint64_t* m);
/* zkhip_prog_assignment, with z in the packed form; the same bytes as zkhip_assignment_pack of its z_out */
int32_t zkhip_prog_assignment_packed(const zkhip_prog* prog, const uint8_t* witness, size_t len, uint8_t* packed_out,
                                     uint64_t cap, uint64_t* packed_len, uint8_t* inputs_out, uint64_t inputs_cap,
                                     uint64_t* n_inputs);
/* zkhip_assignment_upload from the packed form: the same resident assignment, bit for bit */
int32_t zkhip_assignment_upload_packed(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* packed, size_t len,
                                       zkhip_assignment** out);

/* ---- witness files on the device ----
 * A prover service is handed ZoKrates `witness` files.  zkhip_prog_assignment turns one into z on one host thread: it tests every
 * value against r, builds an id -> entry table and gathers m x 32 B into ark order.  The file is fixed-width (u64 count, then
 * count x (i64 id, 32-byte canonical LE value)) and the program's column order is known once the program is parsed, so the same
 * work is a table lookup and a gather, and the device can do it beside the previous proof: the file's bytes are copied as they are
 * (40 B per entry instead of 32 B per variable) and two launches test, order and check them.  Nothing here is a default: the
 * callers choose the route (DESIGN.md section 3 has the measurement).
 *
 * The plan.  zkhip_wplan_create builds, from the program's variable order, two u32 tables — ZoKrates id -> column for ids >= 0 and
 * for ids < 0, each as long as the largest id the program names, "no column" elsewhere — and uploads them; on the host it keeps where
 * the public inputs sit in z: the public arguments in argument order, then ~out_0 .. ~out_{R-1}, R = the program's return count
 * (zkhip_prog_dims [4]), every one an instance column.  It refuses, with ZKHIP_ERR_BAD_ARG and a message that names the reason: an
 * `r1cs` of another curve, l or w than `prog`; an id that occurs at two columns (the reader's "consumed twice (repeated parameter)"
 * case); a public argument or an output below R that has no column or is not an instance column; an id at or above
 * max(2^20, 64 (l + w)) (the reader's range rule refuses it in any file of about the program's size; it would only size the tables).
 * Callers with such programs keep zkhip_prog_assignment.  The plan is tied to its context and to `r1cs`; it may be freed as soon as
 * the last call that takes it has returned (proofs in flight keep what they need of it), and freed and made again at will.  It
 * enqueues copies, so it is refused while a split proof or a queue is pending, like every upload: make it before the queue is opened.
 *
 * zkhip_assignment_upload_witness returns an ordinary zkhip_assignment, bit for bit the one
 * zkhip_assignment_upload(zkhip_prog_assignment(..)) gives, so every *_resident call, zkhip_r1cs_check and the GM17 entry points work
 * unchanged.  Like zkhip_assignment_upload_packed it waits for its verdict.  inputs_out (may be NULL) receives public_inputs_values,
 * *n_inputs (may be NULL) = public arguments + R; an inputs_cap below that is ZKHIP_ERR_BAD_ARG before anything is enqueued.  The
 * host checks the framing first (len >= 8, len == 8 + 40 count, count below 2^32 - 1: ZKHIP_ERR_PARSE with the reader's messages) and
 * that the plan is this context's (ZKHIP_ERR_BAD_ARG).  The context keeps one device buffer for the file's bytes and one u32 per
 * variable, as large as the largest file and system it has seen, until zkhip_ctx_free.
 *
 * Errors are the host reader's wherever the reader defines them:
 *   a value >= r in ANY entry        ZKHIP_ERR_PARSE        "non-canonical field element in the witness"
 *   an id out of range in ANY entry  ZKHIP_ERR_PARSE        "variable id out of range in the witness"  (index — id, or -(id + 1) — at or
 *                                                           above min(2^31, max(2^20, 64 count)))
 *   a variable without a value       ZKHIP_ERR_UNSATISFIED  "assignment missing for variable <name>", the variable of the LOWEST missing
 *                                                           column in the reader's spelling (_k, ~out_k)
 * A PARSE condition wins over a missing variable.  When a file has both PARSE conditions the message is that of the non-canonical
 * value, wherever the two entries are (the reader reports whichever comes first in the file).  Of several entries with one id the last
 * in file order wins, as in the reader; column 0 is 1 whatever the file says about ~one.
 *
 * ONE difference from the host reader: entries for variables the system does not have are ignored (they are still tested against r
 * and the range rule) — negative ids at or above R among them — and the inputs are always the program's public arguments + R outputs,
 * whereas the reader sizes the outputs by the negative ids the file contains.  On a file the reference wrote for the program the two
 * agree. */
typedef struct zkhip_wplan zkhip_wplan;
int32_t zkhip_wplan_create(zkhip_ctx* ctx, const zkhip_prog* prog, const zkhip_r1cs* r1cs, zkhip_wplan** out);
void zkhip_wplan_free(zkhip_wplan* plan);
int32_t zkhip_assignment_upload_witness(zkhip_ctx* ctx, const zkhip_wplan* plan, const uint8_t* witness, size_t len,
                                        uint8_t* inputs_out, uint64_t inputs_cap, uint64_t* n_inputs, zkhip_assignment** out);

/* ---- witnesses computed on the device ----
 * A host that holds a program and its ARGUMENTS runs `zokrates compute-witness` per proof: the reference's interpreter
 * (/root/reference/zokrates_interpreter/src/lib.rs:30-138) is one thread that walks the statements over a BTreeMap, and its `witness`
 * file is what the calls above then read.  A program is a straight-line list and no control flow depends on a value, so a BATCH of
 * instances executes the same statement at the same time: one work-item per instance, the program compiled once into an instruction
 * stream (csrc/xplan.h), the values in device memory instance-minor (csrc/wexec.cuh).  Opt-in: a prove call, upload or queue that
 * never asks for a plan makes the launches and bytes it made before.  A lone instance runs on one lane and is slow; the route pays in
 * batches (DESIGN.md section 3 has the measurement).
 *
 * The plan.  zkhip_xplan_create walks the statements section of the same `out` bytes `prog` was parsed from a second time, with the
 * combinations RAW (no duplicates merged, no zero coefficients dropped), and compiles them in one pass with the set of variables
 * defined so far — ~one and the arguments at the start; a repeated parameter keeps its last value:
 *   Constraint   `lin` of exactly one raw term with coefficient 1 whose variable is not yet defined: a DEFINE, var = left * right;
 *                otherwise a CHECK, left * right == lin (LinComb::is_assignee, zokrates_ast/src/ir/expression.rs:218-222).  A
 *                combination is the sum over its raw terms, the empty one is 0.  Spans and error annotations are skipped.
 *   Directive    the inputs are evaluated as QuadCombs, the outputs stored (they overwrite a defined variable) and defined.  Solvers:
 *                ConditionEq, Bits(n), Div, Xor, Or, ShaAndXorAndXorAnd, ShaCh, EuclideanDiv, with the input and output counts of
 *                Solver::get_signature (zokrates_ast/src/common/solvers.rs:52-69).  Bits is `to_bits_be` cut to the modulus' bit
 *                length, without the interpreter's out-of-range trial (Interpreter::default()); Div by zero is 1; EuclideanDiv by zero
 *                is quotient 0, remainder n.
 *   Log          skipped.
 * Refused with ZKHIP_ERR_BAD_ARG and a message that names the statement number: a statement that reads a variable nothing has
 * defined yet (the variable in the reader's spelling: _k, ~out_k — the reference would panic there); a solver's wrong input or output
 * count; any other solver — Zir, Ref, Sha256Round, SnarkVerifyBls12377, an unknown name — "... keeps the host interpreter", the
 * solver named.  Refused as well: an `r1cs` of another curve, n, l or w than `prog`; `out` bytes of another curve, constraint count,
 * variable order (hence l, w) or argument list than `prog` — the plan checks that it walked the program `prog` was parsed from.  Bytes
 * that are no program are ZKHIP_ERR_PARSE.  The plan keeps the instruction stream, a pool of coefficients in the kernel's form, the
 * slot of every variable (column j of the R1CS is slot j; a variable the system has no column for — a directive output no constraint
 * mentions — sits at or above m = l + w), the ascending signed ids of every variable the interpreter's Witness would hold (the
 * order of the reference's `witness` file: ~out_1, ~out_0, ~one, _0, ...) and the public-input columns.  Tied to its context (a call
 * with another context's plan is refused); of `r1cs` it keeps what it needs — l, w, the columns — and reads nothing again, so the plan
 * outlives it, and the assignments it delivers fit every system of the same program.  Freed and made again at will; it enqueues copies, so it is refused while a split proof or a queue is pending.
 *   zkhip_xplan_dims: out[0] arguments, [1] statements executed, [2] defines, [3] checks, [4] directives, [5] entries of a witness
 *   file, [6] variables without a column, [7] device bytes of value store per instance
 *
 * zkhip_compute_witness runs `count` instances.  args: count x arguments x 32 B canonical LE.  Each of assignments_out (count
 * handles), witness_out (count x witness_cap_each BYTES), inputs_out (count x inputs_cap_each ELEMENTS of 32 B), first_statement and
 * first_row may be NULL; status (count) may not.  Per instance: status[i] = ZKHIP_OK or ZKHIP_ERR_UNSATISFIED; an ordinary
 * zkhip_assignment — m canonical integers in ark order, column 0 = 1, in a buffer of m + 2, exactly what zkhip_assignment_upload
 * leaves, so every *_resident call, zkhip_queue_submit(z_resident) and zkhip_r1cs_check work unchanged (the caller frees it); the
 * reference's `witness` bytes (u64 count, then (i64 id, 32-byte LE value) by ascending id: the first 8 + 40 x dims[5] bytes of the
 * instance's share, the rest is not touched); public_inputs_values (public arguments in argument order, then ~out_0 ..).  A failed
 * instance gets a NULL handle, a zero-filled file and zero-filled inputs, first_statement[i] = the lowest failing item of the
 * statements section (logs and directives are counted) and first_row[i] = the R1CS row of that constraint, which is what
 * zkhip_r1cs_check names; an instance that ran through has UINT64_MAX in both.
 * Returns ZKHIP_OK if every instance ran through; ZKHIP_ERR_UNSATISFIED if any did not — the others are delivered, as checked proving
 * delivers them, and zkhip_last_error names the first failing instance, its statement and its row.  An argument at or above r:
 * ZKHIP_ERR_PARSE before anything is enqueued, the message names the instance and the argument.  A cap that is too small, a plan of
 * another context or a NULL: ZKHIP_ERR_BAD_ARG.  count == 0 is ZKHIP_OK and touches nothing.  The call works through `count` in
 * chunks (ZKHIP_TUNE_EXEC_CHUNK); the context keeps the buffers of its largest chunk — by default up to half of the free device memory,
 * 32 GiB at most — until zkhip_ctx_free, so a context that shares its device with large keys names a chunk.  The assignments are
 * NOT part of that budget: (m + 2) x 32 B per delivered instance, all of a call's at once (190 GB for 4 096 instances of a program of
 * 1.45 M columns), are the caller's to fit — ask for fewer instances per call, or free each handle after its proof
 * (ZKHIP_ERR_DEVICE / _NOMEM otherwise: no handle is delivered).
 * Call discipline as zkhip_pairing_products: a stream and buffers of its own, no proof slot touched — allowed while a proof queue is
 * open (a service computes the next batch between submits and hands the handles to zkhip_queue_submit), refused while a split proof
 * is pending.  Nothing consults the environment.
 *
 * A lone witness across the device (ZKHIP_TUNE_EXEC_WIDE = 1; off by default).  The same call, plan, stream, store, verdicts, gather
 * and file kernels and the same bytes out; one work-item per (instruction of a level, instance) instead of one per instance.  The plan
 * knows which slots every instruction reads and writes, so it also holds the program's dependency LEVELS, computed once on the
 * host when the plan is made: an instruction sits at the lowest level above the last write of every slot it reads and above the last
 * write and every reader of the slots it writes (a directive's output that overwrites a defined variable, the second binding of a
 * repeated parameter: strictly after every reader of the old value); the instructions of one level run in no order.  The call cuts the
 * levels, in ascending order, into launches: a level of ZKHIP_TUNE_EXEC_WIDE_MIN instructions or more is one launch over the whole
 * device, every maximal run of narrower levels one launch of one workgroup per instance with a workgroup barrier between levels.  The
 * stream orders the launches; no launch waits on another workgroup of itself.  The verdict of an instance is the minimum over its
 * failing statements — still "the lowest failing statement".  A program gains what its depth allows: a deep, narrow one stays a chain.
 * Measured: a lone witness of a synthetic program of 2^20 statements in 5 535 levels takes 1.94 s against 12.2 s
 * on one lane; up to 1 024 instances the one-lane route did not win back.
 *   zkhip_xplan_levels: out[0] levels, [1] instructions of the widest level, [2] instructions in all (the arguments' included),
 *   [3] levels of fewer than 64 instructions.  Read-only, no device work.
 *   zkhip_exec_last: the last zkhip_compute_witness of the context that reached the device: out[0] 0 none yet, 1 one work-item per
 *   instance, 2 level-scheduled; [1] chunks; [2] program launches per chunk (1 on route 1; on route 2 the launches the levels were cut
 *   into — one small launch before them writes ~one and the verdict words and is not counted); [3] the WIDE_MIN in force.  Read-only.
 * NULL arguments of either are ZKHIP_ERR_BAD_ARG. */
typedef struct zkhip_xplan zkhip_xplan;
int32_t zkhip_xplan_create(zkhip_ctx* ctx, const zkhip_prog* prog, const zkhip_r1cs* r1cs, const uint8_t* out_bytes, size_t len, zkhip_xplan** out);
void zkhip_xplan_free(zkhip_xplan* plan);
int32_t zkhip_xplan_dims(const zkhip_xplan* plan, uint64_t out[8]);
int32_t zkhip_xplan_levels(const zkhip_xplan* plan, uint64_t out[4]);
int32_t zkhip_exec_last(const zkhip_ctx* ctx, uint64_t out[4]);
int32_t zkhip_compute_witness(zkhip_ctx* ctx, const zkhip_xplan* plan, uint32_t count, const uint8_t* args, zkhip_assignment** assignments_out,
                              uint8_t* witness_out, uint64_t witness_cap_each, uint8_t* inputs_out, uint64_t inputs_cap_each, int32_t* status,
                              uint64_t* first_statement, uint64_t* first_row);

/* Steady-state variant for proofs/sec: `count` assignments (each m x 32 B, contiguous), `count`
 * (r, s) pairs (64 B each) and `count` proof slots (8*sz(Fq)+3 B each).  Same results as `count`
 * calls of zkhip_prove_g16; two proofs are kept in flight, so the latency-bound tail of one proof
 * overlaps the MSMs of the next (timings: per-phase sums over the batch, total_ms = wall clock). */
int32_t zkhip_prove_g16_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count,
                              const uint8_t* z, const uint8_t* rs, uint8_t* proofs_out, zkhip_timings* timings);
/* The same over assignments already resident in HBM (zs[i] may repeat). */
int32_t zkhip_prove_g16_resident_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count,
                                       zkhip_assignment* const* zs, const uint8_t* rs, uint8_t* proofs_out,
                                       zkhip_timings* timings);

/* ---- checked proving ----
 * A prove call turns ANY assignment into proof bytes: one that does not satisfy the system gives a proof that does not verify, and
 * finding that out with the verifier costs a host pairing per proof.  The device holds Az, Bz and Cz before the first transform
 * (over a key bound to the system: Az and Bz, and C's mat-vec is a third of the witness map's), so it can say so itself, and name
 * the constraint — for a program read by zkhip_prog_parse the row is the statement number of the `out` file. */
/* Az o Bz == Cz on the device.  z: host assignment (m x 32 B) or NULL to use z_resident.  ZKHIP_OK and
 * *first_row = UINT64_MAX, *n_bad = 0 when every constraint holds; otherwise ZKHIP_ERR_UNSATISFIED, the lowest
 * failing row and the number of failing rows (either pointer may be NULL).  Works for any key state and scheme:
 * it needs no key. */
int32_t zkhip_r1cs_check(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident,
                         uint64_t* first_row, uint64_t* n_bad);
/* Checked mode of a context (default 0).  Returns the previous setting; on = -1 only reports.
 * In checked mode zkhip_prove_g16, _resident, _batch, _resident_batch and zkhip_prove_gm17, _resident, _resident_batch test
 * every proof's assignment on the device (one pointwise pass over the three row-product vectors; over a bound key C's mat-vec
 * as well) with no further synchronisation.  If any fails, the call returns ZKHIP_ERR_UNSATISFIED, zkhip_last_error names the
 * first failing proof and its constraint, the output slot of every failing proof is zero-filled, the slot of every other proof
 * of the call holds the bytes the unchecked call writes, and the context stays usable.  (on >= 0 while a split proof is pending:
 * ZKHIP_ERR_BAD_ARG, nothing changed.)  With checked mode off nothing changes:
 * the same launches, bytes and return codes as without this section.
 * The multi-GPU entry points — zkhip_prove_*_partial, zkhip_prove_g16_split_*, zkhip_prove_*_multi* — IGNORE checked mode (the
 * members of a zkhip_multi are created with it off): their callers use zkhip_r1cs_check. */
int32_t zkhip_ctx_set_checked(zkhip_ctx* ctx, int32_t on);
/* After a prove call that returned ZKHIP_ERR_UNSATISFIED: up to cap (proof index within the call, first failing
 * row, failing rows) triples, in proof order; *count = how many proofs of the call failed. */
int32_t zkhip_ctx_unsatisfied(const zkhip_ctx* ctx, uint32_t cap, uint32_t* proof_idx, uint64_t* first_row,
                              uint64_t* n_bad, uint32_t* count);

/* ---- proof queue: proofs in flight across calls ----
 * The *_batch calls reach their rate by keeping ZKHIP_TUNE_SLOTS proofs in flight, and drain that pipeline before they return.  A
 * prover service receives its witnesses one at a time: a queue over one (context, key, constraint system) lets it submit each as
 * it arrives and collect the oldest when it wants it — the same pipeline, kept full by the caller.  The scheme is the key's (Groth16
 * or GM17); whole keys only (a shard is refused); one queue per context.  The contract is in Conventions above.
 *   submit        : exactly one of z (m x 32 B, host memory) and z_resident; rnd = r | s (64 B, Groth16) or d1 | d2 | r (96 B, GM17);
 *                   *ticket (may be NULL) = the proof's number.  No host synchronisation.
 *   submit_packed : the assignment in the packed form of zkhip_assignment_pack, validated on the host like
 *                   zkhip_assignment_upload_packed and widened on the device into the proof's own buffer; unlike that upload it does not
 *                   wait for the device: whether every 32-byte value is below r is read when the ticket is collected
 *   submit_witness: the assignment as the bytes of a ZoKrates `witness` file, ordered on the device through `plan` (section "witness files
 *                   on the device") into the proof's own buffer.  The framing and the plan are checked on the host first (a refusal
 *                   consumes no ticket); what the device finds — a value >= r, an id out of range, a missing variable — is read when the
 *                   ticket is collected, with the errors of zkhip_assignment_upload_witness.  No host synchronisation
 *   ready         : never blocks.  *ready = 1 if the OLDEST proof in flight is done on the device (collect will not wait), 0 if it is
 *                   not or the queue is empty
 *   collect       : the oldest proof; blocks until it is done.  *ticket (may be NULL) = its number, proof_out as zkhip_prove_g16,
 *                   timings optional (total_ms: from submit to the end of collect)
 *   collect_inputs: collect, and the public inputs of a ticket that was submitted as a witness file: inputs_out (may be NULL; inputs_cap
 *                   elements of 32 B) and *n_inputs = public arguments + return count.  A ticket from another source gives *n_inputs = 0.
 *                   An inputs_cap that is too small is ZKHIP_ERR_BAD_ARG and spends no ticket.  Plain collect on a witness ticket works and
 *                   drops the inputs
 *   close         : waits for what is in flight, discards it, frees q.  The context is an ordinary context again. */
typedef struct zkhip_queue zkhip_queue;
int32_t zkhip_queue_open(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_queue** out);
int32_t zkhip_queue_state(const zkhip_queue* q, uint32_t* capacity, uint32_t* in_flight);
int32_t zkhip_queue_submit(zkhip_queue* q, const uint8_t* z, zkhip_assignment* z_resident, const uint8_t* rnd, uint64_t* ticket);
int32_t zkhip_queue_submit_packed(zkhip_queue* q, const uint8_t* packed, size_t len, const uint8_t* rnd, uint64_t* ticket);
int32_t zkhip_queue_submit_witness(zkhip_queue* q, const zkhip_wplan* plan, const uint8_t* witness, size_t len, const uint8_t* rnd,
                                   uint64_t* ticket);
int32_t zkhip_queue_ready(zkhip_queue* q, int32_t* ready);
int32_t zkhip_queue_collect(zkhip_queue* q, uint64_t* ticket, uint8_t* proof_out, zkhip_timings* timings);
int32_t zkhip_queue_collect_inputs(zkhip_queue* q, uint64_t* ticket, uint8_t* proof_out, uint8_t* inputs_out, uint64_t inputs_cap,
                                   uint64_t* n_inputs, zkhip_timings* timings);
int32_t zkhip_queue_close(zkhip_queue* q);

/* ---- one proof across several GPUs ----
 * Every MSM is a sum over independent (scalar, base) pairs, so rank k of `world` loads only its index range of
 * a_query / b_g1_query / b_g2_query / l_query / h_query (zkhip_pk_load_g16_shard), computes the partial sums of the five
 * MSMs over that range (zkhip_prove_g16_partial; the mat-vec / NTT stage is replicated on every rank, it is < 10 % of
 * the work) and the ranks exchange ONE fixed-size record each (zkhip_partial_size bytes: five points in XYZZ
 * coordinates) — an all-gather over RCCL in zokrates_amd/parallel.py.  zkhip_combine_g16 adds the records and
 * assembles the proof; the result is bit-identical to zkhip_prove_g16 with the whole key. */
int32_t zkhip_pk_load_g16_shard(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, uint32_t rank,
                                uint32_t world, zkhip_pk** out);
int32_t zkhip_partial_size(int32_t curve, uint64_t* bytes);
/* z: host assignment (m x 32 B) or NULL to use the resident one */
int32_t zkhip_prove_g16_partial(zkhip_ctx* ctx, const zkhip_pk* pk_shard, const zkhip_r1cs* r1cs, const uint8_t* z,
                                zkhip_assignment* z_resident, const uint8_t* r, const uint8_t* s, uint8_t* partial_out,
                                zkhip_timings* timings);
/* partials: count x zkhip_partial_size bytes, one record per rank, any order; pk: any shard (or the whole key) */
int32_t zkhip_combine_g16(zkhip_ctx* ctx, const zkhip_pk* pk, uint32_t count, const uint8_t* partials, const uint8_t* r,
                          const uint8_t* s, uint8_t* proof_out);

/* ---- primitives (exported for parity tests and micro-benchmarks) ---- */
/* [UPSTREAM] ark_poly::Radix2EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place (App. A.4).
 * data: 2^log_n x 32 B canonical LE, natural order in and out, transformed in place.
 * dir: 0 fft, 1 ifft, 2 coset_fft, 3 coset_ifft. */
int32_t zkhip_ntt(zkhip_ctx* ctx, int32_t curve, uint32_t log_n, int32_t dir, uint8_t* data);
/* LibsnarkReduction::witness_map (App. A.3): h coefficients (N x 32 B, natural order). */
int32_t zkhip_witness_map(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, uint8_t* h_out);
/* [UPSTREAM] ark_ec::msm::VariableBaseMSM::multi_scalar_mul (App. A.5).
 * bases: n affine points in the ark uncompressed encoding (2 x sz(Fq) for G1, 4 x sz(Fq) for G2);
 * scalars: n x 32 B canonical LE; out: affine coords canonical LE + 1 infinity-flag byte. */
int32_t zkhip_msm_g1(zkhip_ctx* ctx, int32_t curve, uint64_t n, const uint8_t* bases, const uint8_t* scalars, uint8_t* out);
int32_t zkhip_msm_g2(zkhip_ctx* ctx, int32_t curve, uint64_t n, const uint8_t* bases, const uint8_t* scalars, uint8_t* out);
/* Element-wise Montgomery field ops on the device (parity tests): op 0 add, 1 sub, 2 mul;
 * field 0 = Fr, 1 = Fq; a, b, out: count x sz(field) canonical LE.
 * field 2 = Fq2 = Fq[u]/(u^2 + BETA) (BETA = 1 for bn128 and bls12_381, 5 for bls12_377), elements c0 then c1, 2 x sz(Fq), with
 * the further ops 3 sqr and 4 inv (of a; 0 -> 0; b is read but not used); field 3 = the same field computed in the MSM kernels'
 * unsaturated limbs, ops 2 and 3 in the accumulation kernel's inlined form, with the further ops 5 mul and 6 sqr (the
 * out-of-line forms of the other kernels), 7 = a * b - a * a with one reduction per component (the fused Y3), and 8, 9, 10 =
 * (3a)(4b), (3a)^2, (3a)(4b) - (3a)(4a) on un-reduced multiples (values up to 6p and 8p: the top of the forms' operand range).
 * fields 4 and 5 (tests only) = Fr and Fq, count x sz(field), computed in the single-field unsaturated limbs of the transform
 * passes and the G1 kernels: op 0 add, 1 sub (bias 2p), 2 mul, 3 sqr, 4 sub (bias 4p), 5 mul and 6 sqr with loose quotient digits
 * (where the field has the room; the plain forms otherwise), 7 = 8a through three doublings and the weak reduction, 8, 9, 10 as
 * field 3's on (3a)(4b), (3a)^2, (3a)(4b) - (3a)(4a), 11 = a - 3b by the one-carry-round numerator of X3, and the butterfly
 * shapes of the transforms, each difference or sum multiplied at once without its carry round: 12 = (a - b) b, 13 = (3a - 7b) a,
 * 14 = (a + b) a, 15 = -a b (lazy negation).  Fields above 5 are refused. */
int32_t zkhip_field_op(zkhip_ctx* ctx, int32_t curve, int32_t field, int32_t op, uint64_t count,
                       const uint8_t* a, const uint8_t* b, uint8_t* out);
/* TESTS ONLY.  One function of the group law (csrc/ec.cuh, bind.cuh, kernels_msm.cuh) element by element on the device, called the
 * way a kernel of the product calls it, on RAW limbs: nothing is converted or reduced on the way in or out.
 * group: 1 (coordinates in Fq) or 2 (Fq2, c0 then c1).  form: 0 = the saturated Montgomery words of the fixed-base kernels and the
 * host (sz(Fq) / 4 words per Fq element), 1 = the unsaturated limbs of the MSM, fold and bind kernels (9 limbs of 29 bits for
 * bn128, 14 of 28 bits for the two BLS curves, one uint32 each).  a, b, out: count x 4 coordinates X, Y, ZZ, ZZZ, each coordinate
 * its limbs back to back; an affine operand or result uses X and Y (results: ZZ = ZZZ = 0).  k: count x 8 words, the scalar
 * (little-endian; ops 16 and 17 read word 0).  flags: one byte per element: bit 0 = the sign of the digit for op 2 (the only place
 * where the product takes `neg` at run time; elsewhere it is a constant of the call, and so here: ops 18 and 19), bit 1 = a is the
 * point at infinity, bit 2 = b is (the operand is overwritten on the device before the function reads it).
 * op (b: A = affine, X = XYZZ, - = unused):
 *    0 xyzz_madd_acc<false>(a, A)    1 xyzz_madd_cold(a, A)    2 xyzz_madd_begin<true> + xyzz_madd_finish<true> (a, A, neg; the
 *    caller's precondition: a finite, the x coordinates differ; see the note below)    3 xyzz_add_acc(a, X)    4 xyzz_add_from(a, &X)
 *    5 xyzz_add(a, X)    6 xyzz_add_to(&a, &X)    7 xyzz_dbl    8 xyzz_dbl_inl    9 xyzz_dbl_acc    10, 11 xyzz_dbl_affine_inl<false>,
 *    <true> (a affine)    12 xyzz_neg_u    13 xyzz_to_affine    14 xyzz_to_affine_u    15 xyzz_mul_words(&a, k, 8)
 *    16 xyzz_mul_u32(a, k[0])    17 xyzz_mul_small(a, k[0])    18 xyzz_madd_acc<false>(a, A, true)    19 xyzz_add_from(a, &X, true)
 * Form 0 has ops 0, 5, 6, 7, 13, 16; form 1 the others, 12, 14, 15 and 19 for group 1 only (the kernels that call them exist for G1).
 * Op 2 is the one op NO kernel calls in this form: k_msm_accum carries its own inlined copy of the addition proper (over G1 with X1
 * kept un-reduced below 10p, Pp against 16p and no weak reduction of X3), which only MSMs and proofs reach; op 2 holds the two
 * functions as ec.cuh defines them, with the hot products.
 * Preconditions are the functions' own (operand bounds as written in ec.cuh); the call checks ids and pointers only and refuses
 * every other (group, form, op). */
int32_t zkhip_group_op(zkhip_ctx* ctx, int32_t curve, int32_t group, int32_t form, int32_t op, uint64_t count,
                       const uint32_t* a, const uint32_t* b, const uint32_t* k, const uint8_t* flags, uint32_t* out);

/* ---- the pairing check on the device (csrc/pairing.cuh) ----
 * The device counterpart of the host layer's `pairing_product_is_one` (csrc/host/verify.cpp), and the primitive under the check
 * the reference makes in `<Ark as Backend<T, G16>>::verify` (/root/reference/zokrates_ark/src/groth16.rs:55-87: ark_groth16's
 * e(A, B) e(-g_ic, gamma) e(-C, delta) e(-alpha, beta) == 1) and in `<Ark as Backend<T, GM17>>::verify` (gm17.rs:69-110: two such
 * products): ok_out[i] = 1 iff prod_k e(g1[i][k], g2[i][k]) == 1, for count independent items of pairs_per_item (1 .. 8) pairs each.
 * Deterministic, one verdict per item; no random linear combination.
 *   g1     : count x pairs_per_item records of 2 x sz(Fq) + 1 bytes: x, y canonical LE and a flag byte (non-zero: the point at
 *            infinity), the record of A and C in proof_out of zkhip_prove_g16
 *   g2     : the same with 4 x sz(Fq) + 1 bytes: x.c0 x.c1 y.c0 y.c1 and the flag byte
 *   ok_out : count bytes, 0 or 1
 * A pair with a point at infinity contributes 1 (the host verifier's product skips it).  A point that is not on its curve / twist
 * or not in the r-torsion makes its item's verdict 0 (tested on the device: r P = O by the group law of csrc/ec.cuh; bn128's G1 has
 * cofactor 1).  A coordinate that is not below the field modulus is the caller's error: ZKHIP_ERR_PARSE, the message names the
 * lowest such item, and ok_out is not written.  count == 0 is ZKHIP_OK and touches nothing.
 * The call runs on a stream and in buffers of its own and touches no proof slot: it is allowed while a proof queue is open (to
 * check collected proofs between submits) and refused, like every other call, while a split proof is pending. */
int32_t zkhip_pairing_products(zkhip_ctx* ctx, int32_t curve, uint64_t count, uint32_t pairs_per_item,
                               const uint8_t* g1, const uint8_t* g2, uint8_t* ok_out);
/* ---- verify on the device: one verdict per proof ----
 * Replaces `<Ark as Backend<T, G16>>::verify` (/root/reference/zokrates_ark/src/groth16.rs:55-87: ark_groth16::verify_proof) and
 * `<Ark as Backend<T, GM17>>::verify` (gm17.rs:69-110: ark_gm17::verify_proof) for batches of proofs under one key; for every input
 * on which the host layer's `verify` answers true or false the verdict is the same, and where it throws the call fails.
 * zkhip_vk_load_*: `bytes` is ark's VerifyingKey in the `serialize_unchecked` layout — g16: alpha_g1, beta_g2, gamma_g2, delta_g2,
 * gamma_abc_g1[]; gm17: h_g2, g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, query[] — which is the head of a `proving.key`, so a
 * whole proving key is accepted too.  Every point of the key is tested on the device like a proof point (canonical coordinates, on
 * its curve / twist, r P = O); a key with a point that fails, a point at infinity or too few bytes is refused with
 * ZKHIP_ERR_PARSE.  What depends on the key alone is prepared here (the negated points, every point in the kernels' limbs).
 * zkhip_vk_dims: out[0] = l, the number of public inputs (points of gamma_abc / query less one), out[1] = 0 Groth16, 1 GM17. */
int32_t zkhip_vk_load_g16(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_vk** out);
int32_t zkhip_vk_load_gm17(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_vk** out);
void zkhip_vk_free(zkhip_vk* vk);
int32_t zkhip_vk_dims(const zkhip_vk* vk, uint64_t out[2]);
/*   proofs : count records in exactly the proof_out layout of zkhip_prove_g16 / zkhip_prove_gm17 (8 x sz(Fq) + 3 bytes)
 *   inputs : count x l x 32 B, canonical LE (may be NULL when l == 0)
 *   ok_out : count bytes, 0 or 1
 * g_ic = gamma_abc[0] + sum_i input_i gamma_abc[i + 1] is computed per proof on the device, for any l.  A point of a proof that is
 * off its curve, outside the r-torsion or flagged as the point at infinity makes that proof's verdict 0, as on the host.  A
 * coordinate that is not below the field modulus or an input that is not below r is the host verifier's Error: ZKHIP_ERR_PARSE,
 * the message names the lowest such item and the value, and no verdict is written.  A key of the other scheme, of another context,
 * or a NULL pointer: ZKHIP_ERR_BAD_ARG.  count == 0 is ZKHIP_OK and touches nothing.  Call discipline as zkhip_pairing_products:
 * allowed while a proof queue is open, refused while a split proof is pending; nothing consults the environment. */
int32_t zkhip_verify_g16_batch(zkhip_ctx* ctx, const zkhip_vk* vk, uint64_t count, const uint8_t* proofs, const uint8_t* inputs,
                               uint8_t* ok_out);
int32_t zkhip_verify_gm17_batch(zkhip_ctx* ctx, const zkhip_vk* vk, uint64_t count, const uint8_t* proofs, const uint8_t* inputs,
                                uint8_t* ok_out);
/* TESTS ONLY.  One function of the Fq12 arithmetic of csrc/pairing.cuh per call, item by item, on RAW limbs in the layout of the
 * pairing kernel (one group of lanes per item, the values in LDS): nothing is converted or reduced on the way in or out.
 * Fq12 = Fq2[w] / (w^6 - xi); a, b, out: count x 6 coefficients (of w^0 .. w^5) x 2 components (c0, c1) x N limbs, N = 9 limbs of
 * 29 bits for bn128, 14 of 28 bits for the BLS curves, Montgomery form with respect to 2^(N x bits).  Operands: every limb at most
 * 2^bits + 8 and every value below 3p, the bound the kernel keeps; results obey the same.
 * op: 0 a b   1 a^2   2 a times the line whose three values are b's coefficients at the line's positions (w^0, w^1, w^3 on the type D
 * twists of bn128 and bls12_377; w^0, w^2, w^3 on bls12_381's type M twist; b's other coefficients are not read)   3 1 / a (0 -> 0)
 * 4 a^p   5 a^(p^6).  b is read for every op. */
int32_t zkhip_tower_op(zkhip_ctx* ctx, int32_t curve, int32_t op, uint64_t count, const uint32_t* a, const uint32_t* b, uint32_t* out);

/* ---- "next" row N3: setup ----
 * Replaces `Groth16::<E>::circuit_specific_setup` at /root/reference/zokrates_ark/src/groth16.rs:95
 * ([UPSTREAM] generate_random_parameters, App. A.6) with the randomness made explicit:
 * toxic = alpha, beta, gamma, delta, tau (5 x 32 B); g1/g2 = group generators in ark uncompressed
 * encoding (ark samples random ones; NULL = the standard generators).  Writes the ark
 * `serialize_unchecked` proving key into pk_out (size from zkhip_setup_g16_size). */
int32_t zkhip_setup_g16_size(const zkhip_r1cs* r1cs, uint64_t* pk_bytes);
int32_t zkhip_setup_g16(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* toxic, const uint8_t* g1,
                        const uint8_t* g2, uint8_t* pk_out, uint64_t pk_cap);

/* ---- GM17: the second proof system behind the same Backend trait (BASELINE.json config 5) ----
 * Replaces `<Ark as Backend<T, GM17>>::generate_proof` (/root/reference/zokrates_ark/src/gm17.rs:43-78):
 * zkhip_pk_load_gm17 stands for `ProvingKey::deserialize_unchecked` (:60-62) — `bytes` is the `proving.key` written by
 * the reference's GM17 `setup` (:27-28; [UPSTREAM] ark_gm17::ProvingKey in `serialize_unchecked` layout: vk{h_g2,
 * g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, query[]}, a_query[], b_query[] (G2), c_query_1[], c_query_2[],
 * g_gamma_z, h_gamma_z (G2), g_ab_gamma_z, g_gamma2_z2, g_gamma2_z_t[]) — and zkhip_prove_gm17 for `GM17::prove`
 * (:64; [UPSTREAM] ark_gm17::create_random_proof).  The constraint system is the same zkhip_r1cs (the R1CS -> SAP
 * reduction happens on the device); the assignment is the same m x 32 B vector in ark order.
 *   d1_d2_r  : the three blinding scalars (3 x 32 B) in the order ark samples them (`Fr::rand(rng)` x 3: d1, d2, r)
 *   proof_out: as zkhip_prove_g16 (A | B | C canonical LE + 3 infinity flags); zkhip_pk_dims gives out[0] = SAP
 *              variables (a_query len), out[1] = g_gamma2_z_t len, out[2] = c_query_1 len, out[3] = query len. */
int32_t zkhip_pk_load_gm17(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_pk** out);
int32_t zkhip_prove_gm17(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, const uint8_t* d1_d2_r,
                         uint8_t* proof_out, zkhip_timings* timings);
int32_t zkhip_prove_gm17_resident(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_assignment* z,
                                  const uint8_t* d1_d2_r, uint8_t* proof_out, zkhip_timings* timings);
/* `count` proofs, two in flight (see zkhip_prove_g16_resident_batch); d1_d2_r: count x 96 B. */
int32_t zkhip_prove_gm17_resident_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count,
                                        zkhip_assignment* const* zs, const uint8_t* d1_d2_r, uint8_t* proofs_out,
                                        zkhip_timings* timings);
/* One GM17 proof across several GPUs, exactly as for Groth16 (zkhip_pk_load_g16_shard ...): rank k loads its index range of
 * a_query / b_query / c_query_1 / c_query_2 / g_gamma2_z_t, computes the five partial sums over it, the ranks exchange one
 * zkhip_partial_size-byte record each, zkhip_combine_gm17 adds them and assembles the proof (bit-identical). */
int32_t zkhip_pk_load_gm17_shard(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, uint32_t rank,
                                 uint32_t world, zkhip_pk** out);
int32_t zkhip_prove_gm17_partial(zkhip_ctx* ctx, const zkhip_pk* pk_shard, const zkhip_r1cs* r1cs, const uint8_t* z,
                                 zkhip_assignment* z_resident, const uint8_t* d1_d2_r, uint8_t* partial_out,
                                 zkhip_timings* timings);
int32_t zkhip_combine_gm17(zkhip_ctx* ctx, const zkhip_pk* pk, uint32_t count, const uint8_t* partials,
                           const uint8_t* d1_d2_r, uint8_t* proof_out);
/* Replaces `GM17::circuit_specific_setup` at /root/reference/zokrates_ark/src/gm17.rs:25 ([UPSTREAM]
 * ark_gm17::generate_parameters) with the randomness explicit: toxic = alpha, beta, gamma, t (4 x 32 B; ark's
 * generate_random_parameters fixes gamma = 1); g1/g2 as in zkhip_setup_g16. */
int32_t zkhip_setup_gm17_size(const zkhip_r1cs* r1cs, uint64_t* pk_bytes);
int32_t zkhip_setup_gm17(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* toxic, const uint8_t* g1,
                         const uint8_t* g2, uint8_t* pk_out, uint64_t pk_cap);

/* ---- one proof across several GPUs of ONE process (§8b "multi-GPU handled inside one context") ----
 * A caller behind the reference's trait (`Backend::generate_proof`, /root/reference/zokrates_proof_systems/src/lib.rs:98-112,
 * call site /root/reference/zokrates_cli/src/ops/generate_proof.rs:187) is a single process without a collective
 * library; zkhip_multi gives it the latency mode of the sharded entry points above without one.  It owns one context
 * per listed device (a device may be listed more than once: the members then share it, which is how the path is tested
 * on a one-GPU box), member k holds shard k of n of the proving key (1/n of every base table) and a replica of the
 * constraint system.  zkhip_prove_*_multi runs the members' shares on one host thread each — assignment upload,
 * replicated mat-vec / NTT stage, the five MSMs over the member's index ranges — collects the n canonical partial
 * records (zkhip_partial_size bytes each, produced in host memory: nothing larger ever has to cross between devices)
 * and assembles the proof on the calling thread.  The result is bit-identical to the single-GPU proof.
 * zkhip_multi_ctx lends a member's context (e.g. to run zkhip_setup_g16 on member 0); errors of the zkhip_multi_* /
 * zkhip_prove_*_multi calls are reported by zkhip_multi_last_error. */
typedef struct zkhip_multi zkhip_multi;
int32_t zkhip_ctx_create_multi(const int32_t* devices, int32_t n, zkhip_multi** out);
void zkhip_multi_free(zkhip_multi* m);
int32_t zkhip_multi_size(const zkhip_multi* m);
zkhip_ctx* zkhip_multi_ctx(zkhip_multi* m, int32_t member);
/* The exchange step of zkhip_prove_*_multi over RCCL instead of host memory (BASELINE.json's "RCCL ...
 * over xGMI"): on != 0 creates one RCCL communicator per member (ncclCommInitAll; librccl.so.1 is bound with dlopen at
 * this call, libzkhip does not link it) and from then on every member leaves the bucket-set sums of its five partial
 * MSMs on its device and the members ncclAllGather them (two small messages per proof, latency-bound); member 0's copy
 * is read back and combined into the same proof bytes.  Needs distinct devices (ZKHIP_ERR_BAD_ARG otherwise: RCCL
 * refuses two ranks on one GPU) and a loadable librccl (ZKHIP_ERR_DEVICE); on failure the host exchange stays in use.
 * zkhip_multi_exchange describes the exchange in use (RCCL version and rank count, or the host path). */
int32_t zkhip_multi_use_rccl(zkhip_multi* m, int32_t on);
const char* zkhip_multi_exchange(const zkhip_multi* m);
const char* zkhip_multi_last_error(const zkhip_multi* m);
int32_t zkhip_multi_r1cs_load(zkhip_multi* m, int32_t curve, uint64_t n, uint64_t l, uint64_t w, const uint64_t* rowptr_a,
                              const uint32_t* col_a, const uint8_t* val_a, const uint64_t* rowptr_b, const uint32_t* col_b,
                              const uint8_t* val_b, const uint64_t* rowptr_c, const uint32_t* col_c, const uint8_t* val_c);
int32_t zkhip_multi_pk_load_g16(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len);
int32_t zkhip_multi_pk_load_gm17(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len);
int32_t zkhip_prove_g16_multi(zkhip_multi* m, const uint8_t* z, const uint8_t* r, const uint8_t* s, uint8_t* proof_out,
                              zkhip_timings* timings);
int32_t zkhip_prove_gm17_multi(zkhip_multi* m, const uint8_t* z, const uint8_t* d1_d2_r, uint8_t* proof_out,
                               zkhip_timings* timings);
/* Throughput mode of the same object (SURVEY.md §8e "replicas"): zkhip_multi_pk_load_g16_replicas puts the WHOLE key on every
 * member, zkhip_prove_g16_multi_batch splits `count` independent proofs (z: count x m x 32 B, rs: count x 64 B = r | s,
 * proofs_out: count x proof bytes) into one contiguous block per member and runs the members' pipelined batch calls on
 * one host thread each — no communication at all; what a long-lived prover service behind the trait would call. */
int32_t zkhip_multi_pk_load_g16_replicas(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len);
/* The members' keys (shards or replicas, Groth16 or GM17) bound to the members' constraint system — see zkhip_pk_bind_r1cs below;
 * `key_bytes` = the key file the members were loaded from.  All members or none. */
int32_t zkhip_multi_bind(zkhip_multi* m, const uint8_t* key_bytes, size_t len);
int32_t zkhip_multi_unbind(zkhip_multi* m);
/* The witness map of ONE proof split between the members (north_star: "NTT domain shard"): over keys bound to the
 * system a proof needs a and b on the coset and nothing else of the witness map, so members of even rank transform a, members of odd
 * rank b (two transforms each instead of four), partners copy each other's vector — N x 32 bytes device to device (xGMI peer copy
 * between GPUs) — and every member forms the products of its own index range.  On by default for Groth16 members that are bound
 * (zkhip_multi_bind) over domains of at least 2^18 (ZKHIP_SPLIT_MIN_LOG; below, two small transforms cost less than the exchange);
 * every other case runs the whole map on every member, as SURVEY.md §8e recommends for it.  Same proof bytes either way.
 * zkhip_multi_transform_split(m, 0 / 1) switches it (-1: leave it), returning the previous setting; zkhip_multi_last_split tells
 * whether the last zkhip_prove_*_multi did split. */
int32_t zkhip_multi_transform_split(zkhip_multi* m, int32_t on);
int32_t zkhip_multi_last_split(const zkhip_multi* m);
/* ---- the transform DOMAIN sharded across the members (csrc/ntt_shard.h) ----
 * A plan's domain N = N1 x Nb is an N1 x Nb matrix.  Member k of G runs the outer pass on its strip — columns [k Nb/G, (k+1) Nb/G) —
 * and every other pass on its range — elements [k N/G, (k+1) N/G) —, with ONE all-to-all of N/G x 32 bytes per member between them
 * (packed on the device, copied device to device: xGMI peer copies between GPUs, plain copies between members that share one).
 * A transform shards when G is a power of two >= 2, its plan has at least two passes, G <= N1 and 2 G <= Nb.
 *   zkhip_multi_ntt           zkhip_ntt over the members: same arguments, same bytes out (natural order in and out);
 *   zkhip_multi_witness_map   zkhip_witness_map over the members' constraint system (zkhip_multi_r1cs_load): the same h bytes
 *                             (N x 32 B, natural order); three all-to-alls, the mat-vec replicated on every member.
 * Both shard whenever they can; otherwise member 0 runs the single-context call.  Errors: zkhip_multi_last_error.
 *   zkhip_multi_transform_shard(m, 0 / 1)   lets zkhip_prove_g16_multi shard the witness map of a proof over a Groth16 key that is
 *                             NOT bound to its system (-1: leave it); returns the previous setting.  OFF by default: no machine with
 *                             more than one GPU has measured it.  Bound keys keep the a/b split above, GM17 and whatever does not
 *                             shard stay replicated; the proof bytes are the same on every path.
 *   zkhip_multi_last_shard    the number of members the transforms of the last zkhip_multi_ntt / _witness_map / zkhip_prove_*_multi
 *                             were sharded over (0: they were not).
 * Not sharded: bound keys, GM17, replicas and zkhip_prove_g16_multi_batch, ranks in separate processes (split_begin / _end), member
 * counts that are not powers of two. */
int32_t zkhip_multi_ntt(zkhip_multi* m, int32_t curve, uint32_t log_n, int32_t dir, uint8_t* data);
int32_t zkhip_multi_witness_map(zkhip_multi* m, const uint8_t* z, uint8_t* h_out);
int32_t zkhip_multi_transform_shard(zkhip_multi* m, int32_t on);
int32_t zkhip_multi_last_shard(const zkhip_multi* m);
int32_t zkhip_prove_g16_multi_batch(zkhip_multi* m, uint32_t count, const uint8_t* z, const uint8_t* rs, uint8_t* proofs_out,
                                    zkhip_timings* timings);

/* ---- "next" row N2: proving-key cache ----
 * zkhip_pk_export writes the *resident* form of a loaded key (Groth16 or GM17, whole or one shard): packed Montgomery
 * points, MSM-ready order, the extended base vectors — the bytes the GPU holds, plus a small header.
 * zkhip_pk_import brings such an image back with five (a bound key: seven) host-to-device copies and no parsing or conversion, taking
 * `ProvingKey::deserialize_unchecked` (/root/reference/zokrates_ark/src/groth16.rs:40-42; one Fq multiplication per
 * coordinate and a single-threaded read in the reference) off the per-invocation path.
 * A resident key is a set of five MSM tables: level 0 = the key's points, the further levels their precomputed window
 * multiples.  The image carries level 0 only and the import recomputes the other levels on the device
 * (~0.1 s for a 2^20-constraint key — less than reading them from a disk would take: an image that carried every level was
 * measured 2x slower end to end in round 3 and has been removed).
 * The library does no file I/O: the caller stores the image wherever it likes, keyed e.g. by the SHA-256 of the
 * `proving.key` it came from (`zkhip-cli generate-proof --key-cache DIR` does exactly that).  An image
 * is tied to the library build that wrote it (magic + layout version); a foreign image is rejected with ZKHIP_ERR_PARSE. */
int32_t zkhip_pk_export_size(const zkhip_pk* pk, uint64_t* bytes);
int32_t zkhip_pk_export(const zkhip_pk* pk, uint8_t* out, uint64_t cap);
int32_t zkhip_pk_import(zkhip_ctx* ctx, const uint8_t* bytes, size_t len, zkhip_pk** out);

/* ---- a resident prover's key: bound to its constraint system ----
 * The reference turns the evaluations of a, b, c into the coefficients of h = (ab - c)/Z with seven transforms per proof
 * ([UPSTREAM] ark-groth16 0.3.0 `LibsnarkReduction::witness_map`, reached from `Groth16::prove`,
 * /root/reference/zokrates_ark/src/groth16.rs:44), only to pair the coefficients with `h_query`.  Those transforms are linear,
 * so a prover that keeps a key resident can apply them to the key's BASES once: zkhip_pk_bind_r1cs computes
 *   H'_j = sum_i (g^-i / N) w^(-ij) h_query[i]           (pairs with a(g w^j) b(g w^j) / Z(g), the quotient's evaluations) and
 *   L'_v = l_query[v] + sum_k C[k][v] H''_k              (c's inverse transform and its mat-vec, folded into the l bases)
 * and keeps them beside the key's own tables.  From then on zkhip_prove_g16* with THIS key and THIS constraint system takes four
 * transforms and the mat-vec of A and B only; the proof's group elements — hence its bytes — are the same (the same holds for an
 * assignment that does not satisfy the system: what the reference's MSM over h[..N-1] ignores, the bound bases ignore).  Any
 * other constraint system, and every call after zkhip_pk_unbind, takes the key's own tables.  Costs two size-N transforms
 * over G1 points (about a second at 2^20) and two more MSM tables of device memory (ZKHIP_ERR_NOMEM when they do not fit; the key stays
 * usable, unbound).  A call that is refused for its arguments leaves an earlier binding untouched.
 * GM17 keys bind the same way (/root/reference/zokrates_ark/src/gm17.rs:63: the SAP quotient (U^2 - W)/Z is linear in W and in the
 * last transform): TWO transforms per proof instead of four on the twice-larger SAP domain, W's share on the c_query_1 bases.
 * A SHARD of a multi-GPU key holds only its index ranges of the bases, and the transforms need every base once:
 * zkhip_pk_bind_r1cs_shard takes the key FILE again (the bytes the shard was loaded from), computes H' / L' over the whole range
 * and keeps this shard's ranges (works for a whole key as well); zkhip_multi_bind does it for the members of a zkhip_multi — one
 * member computes, every member installs its ranges.
 * A key image (zkhip_pk_export) of a bound key carries level 0 of H' / L' and a fingerprint of the constraint system
 * (zkhip_r1cs_fingerprint: a position-keyed checksum of the resident matrices — a guard against mix-ups, not a commitment);
 * zkhip_pk_bind_r1cs on the imported key attaches the tables when the fingerprint of `r1cs` agrees — a restart costs a read and a
 * checksum, not the transforms.
 * zkhip_pk_is_bound: 1 if proofs over `r1cs` would take the bound tables, else 0. */
int32_t zkhip_pk_bind_r1cs(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* r1cs);
int32_t zkhip_pk_unbind(zkhip_pk* pk);
int32_t zkhip_pk_bind_r1cs_shard(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* key_bytes, size_t len);
/* The same split for ranks that are separate PROCESSES (one per GPU, torch.distributed / MPI around them): `begin` stages the
 * assignment, starts this rank's MSMs over it and transforms ITS half of the witness map — half = 0: a, 1: b on the coset — into
 * `half_out` (N x 32 bytes of host memory; N = the key's domain); the caller exchanges halves with a rank of the other parity;
 * `end` takes the partner's half and leaves the rank's partial record (as zkhip_prove_g16_partial).  The key must be bound
 * (zkhip_pk_bind_r1cs_shard).  zokrates_amd/parallel.py prove_sharded does exactly this over RCCL / gloo.
 * After a successful `begin` the proof is pending (see Conventions): the context remembers the key, the constraint system and that
 * the key was bound, and `end` finishes THAT proof — it wants the same `pk` and `r1cs` (ZKHIP_ERR_BAD_ARG otherwise, the proof stays
 * pending), and is refused the same way when nothing is pending: without a `begin`, or a second time for a proof already collected.
 * A `begin` that returns an error leaves nothing pending; so does an `end` that fails after its argument checks.  A `begin` that
 * is refused because its key is not bound, its `half` is not 0 or 1, or r / s is not canonical has enqueued nothing.
 * zkhip_prove_g16_split_abort is for the caller that gives the exchange up after `begin` (its partner failed): it waits for what the
 * head enqueued, drops the pending proof and leaves the context as before `begin`; ZKHIP_OK also when nothing is pending. */
int32_t zkhip_prove_g16_split_begin(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident,
                                    const uint8_t* r, const uint8_t* s, int32_t half, uint8_t* half_out);
int32_t zkhip_prove_g16_split_end(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* other_half, uint8_t* partial_out,
                                  zkhip_timings* timings);
int32_t zkhip_prove_g16_split_abort(zkhip_ctx* ctx);
int32_t zkhip_r1cs_fingerprint(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, uint64_t out[2]);
/* How the sparse mat-vec (K1) of a proof over `r1cs` is launched — read-only, no device work; for tests and tools that have to
 * know which path their data takes.  lanes[k]: work-items that share a row of A, B, C in a launch over all three matrices (1, 2,
 * 4, 8 or 16: the largest power of two <= half the average length of the matrix's rows of at most 32 terms, so 16 needs
 * every row to have exactly 32).  n_long: rows of 33 to 512 terms (a wavefront each); n_huge: rows of more than 512 terms (a
 * workgroup each), over the three matrices together.  A launch over fewer matrices (a bound key: A and B; one half of a split
 * proof: one of them) uses the same width for those it runs. */
int32_t zkhip_r1cs_matvec_shape(const zkhip_r1cs* r1cs, int32_t lanes[3], uint64_t* n_long, uint64_t* n_huge);
int32_t zkhip_pk_is_bound(const zkhip_pk* pk, const zkhip_r1cs* r1cs);

/* ---- "next" row N1: ZoKrates' own input files (host only: no context, no device work) ----
 * zkhip_prog_parse replaces `ProgEnum::deserialize` (/root/reference/zokrates_ast/src/ir/serialize.rs:306-390: header,
 * sections, per-statement CBOR) followed by `Computation::generate_constraints`
 * (/root/reference/zokrates_ark/src/lib.rs:80-129): `bytes` is the `out` file `zokrates compile` writes; the result is
 * the R1CS in ark variable order — ONE, then instance variables (public arguments in argument order, `~out_k` as
 * first seen), then witness variables (private arguments, then the others as first seen walking the A, B, C linear
 * combinations of every constraint); duplicate variables in a combination are summed, zero coefficients dropped;
 * directives and logs are ignored.  Errors are reported through zkhip_last_error(NULL).
 *   zkhip_prog_dims: out[0] curve id, [1] n, [2] l, [3] w, [4] return count, [5] public arguments, [6] nnz(A)+nnz(B)+nnz(C)
 *   zkhip_prog_matrix: CSR arrays of A (0), B (1), C (2), valid until zkhip_prog_free — the arguments of zkhip_r1cs_load
 *   zkhip_prog_variable_order: the ZoKrates variable id of every column (0 = ~one, k > 0 = _{k-1}, -k = ~out_{k-1})
 *   zkhip_prog_r1cs_load: zkhip_r1cs_load of those matrices
 * zkhip_prog_assignment replaces `Witness::read` (/root/reference/zokrates_ast/src/ir/witness.rs:55-71) and the
 * `witness.remove(..)` walk of generate_constraints: `witness` is the file `zokrates compute-witness` writes; z_out
 * (m x 32 B, may be NULL) is the assignment in ark order — the `z` of zkhip_prove_g16 — and inputs_out (may be NULL;
 * inputs_cap elements of 32 B) receives `public_inputs_values` (/root/reference/zokrates_ast/src/ir/mod.rs:278-288:
 * public arguments in argument order, then ~out_0, ~out_1, ...: the `inputs` of proof.json); a variable without a value
 * gives ZKHIP_ERR_UNSATISFIED (the reference panics with AssignmentMissing). */
int32_t zkhip_prog_parse(const uint8_t* bytes, size_t len, zkhip_prog** out);
void zkhip_prog_free(zkhip_prog* prog);
int32_t zkhip_prog_dims(const zkhip_prog* prog, uint64_t out[8]);
int32_t zkhip_prog_matrix(const zkhip_prog* prog, int32_t which, const uint64_t** rowptr, const uint32_t** col,
                          const uint8_t** val);
int32_t zkhip_prog_variable_order(const zkhip_prog* prog, const int64_t** ids);
int32_t zkhip_prog_r1cs_load(zkhip_ctx* ctx, const zkhip_prog* prog, zkhip_r1cs** out);
/* The inverse of zkhip_prog_parse: an R1CS (CSR, canonical LE values, m columns) as the bytes of a ZoKrates `out` program
 * whose statements are exactly the constraints in row order — `ProgIterator::serialize`
 * (/root/reference/zokrates_ast/src/ir/serialize.rs:202-279) for a program without directives.  ids[j] is the ZoKrates
 * variable id of column j (0 = ~one, k > 0 = _{k-1}, -k = ~out_{k-1}); (arg_ids, arg_private)[n_args] is the argument
 * list.  A reader numbers variables in first-seen order, so the columns come back in this order only if the rows
 * mention them in it.  `out` must hold zkhip_prog_write_bound(n, nnz(A)+nnz(B)+nnz(C), n_args) bytes; *len = bytes
 * written.  Host only. */
int32_t zkhip_prog_write_bound(uint64_t n, uint64_t nnz, uint64_t n_args, uint64_t* bytes);
int32_t zkhip_prog_write(int32_t curve, uint64_t n, uint64_t m, const uint64_t* rowptr_a, const uint32_t* col_a, const uint8_t* val_a,
                         const uint64_t* rowptr_b, const uint32_t* col_b, const uint8_t* val_b, const uint64_t* rowptr_c,
                         const uint32_t* col_c, const uint8_t* val_c, const int64_t* ids, const int64_t* arg_ids,
                         const uint8_t* arg_private, uint64_t n_args, uint32_t return_count, uint8_t* out, uint64_t cap,
                         uint64_t* len);
int32_t zkhip_prog_assignment(const zkhip_prog* prog, const uint8_t* witness, size_t len, uint8_t* z_out,
                              uint8_t* inputs_out, uint64_t inputs_cap, uint64_t* n_inputs);

/* Library / device description, NUL-terminated, for logs. */
int32_t zkhip_describe(const zkhip_ctx* ctx, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */
