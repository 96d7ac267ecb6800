// core.cuh — host side of libzkhip.so: contexts, key/constraint-system residency and the Groth16 prover
// schedule, templated on the curve.  Instantiated once per curve in curve_bn254.hip / curve_bls381.hip / curve_bls377.hip
// (separate translation units so the curves compile in parallel); the C ABI lives in zkhip_api.hip.
//
// Replaces `<Ark as Backend<T, G16>>::generate_proof` (/root/reference/zokrates_ark/src/groth16.rs:20-53)
// from the point where the reference hands over to ark: `ProvingKey::deserialize_unchecked` (:40-42) and
// `Groth16::prove` (:44).  SURVEY.md §8(a) rows a7, a8, K1-K9.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <unordered_set>
#include <vector>

#include "../../include/zkhip.h"
#include "devrt.h"
#include "ntt_geom.h"
#include "msm_geom.h"
#include "ec.cuh"
#include "kernels_msm.cuh"
#include "kernels_ntt.cuh"
#include "zpack.cuh"
#include "wingest.cuh"
#include "wplan.h"
#include "wexec.cuh"
#include "xplan.h"

namespace zk {

// ------------------------------------------------------------------ curves
struct CurveBn254 {
    static constexpr int ID = ZKHIP_CURVE_BN128;
    typedef Fe<Bn254Fr> Fr;
    typedef Fe<Bn254Fq> Fq;
    typedef Fe2<Bn254Fq> Fq2;
    static constexpr u64 GENERATOR = 5;       // Fr::GENERATOR, the coset shift g
    static constexpr int TWO_ADICITY = 28;
    // standard generators, canonical limbs (G1: x, y; G2: x.c0, x.c1, y.c0, y.c1); BN254's are the ones pinned by
    // /root/reference/zokrates_proof_systems/src/solidity.rs:430-441
    static const u32* g1_gen() { static const u32 t[] = {0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}; return t; }
    static const u32* g2_gen() { static const u32 t[] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu, 0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u, 0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u, 0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}; return t; }
};
struct CurveBls381 {
    static constexpr int ID = ZKHIP_CURVE_BLS12_381;
    typedef Fe<Bls381Fr> Fr;
    typedef Fe<Bls381Fq> Fq;
    typedef Fe2<Bls381Fq> Fq2;
    static constexpr u64 GENERATOR = 7;
    static constexpr int TWO_ADICITY = 32;
    // standard generators, canonical limbs (G1: x, y; G2: x.c0, x.c1, y.c0, y.c1); BN254's are the ones pinned by
    // /root/reference/zokrates_proof_systems/src/solidity.rs:430-441
    static const u32* g1_gen() { static const u32 t[] = {0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu, 0x2695638cu, 0x3197d794u, 0x17f1d3a7u, 0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u, 0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u}; return t; }
    static const u32* g2_gen() { static const u32 t[] = {0xc121bdb8u, 0xd48056c8u, 0xa805bbefu, 0x0bac0326u, 0x7ae3d177u, 0xb4510b64u, 0xfa403b02u, 0xc6e47ad4u, 0x2dc51051u, 0x26080527u, 0xf08f0a91u, 0x024aa2b2u, 0x5d042b7eu, 0xe5ac7d05u, 0x13945d57u, 0x334cf112u, 0xdc7f5049u, 0xb5da61bbu, 0x9920b61au, 0x596bd0d0u, 0x88274f65u, 0x7dacd3a0u, 0x52719f60u, 0x13e02b60u, 0x08b82801u, 0xe1935486u, 0x3baca289u, 0x923ac9ccu, 0x5160d12cu, 0x6d429a69u, 0x8cbdd3a7u, 0xadfd9baau, 0xda2e351au, 0x8cc9cdc6u, 0x727d6e11u, 0x0ce5d527u, 0xf05f79beu, 0xaaa9075fu, 0x5cec1da1u, 0x3f370d27u, 0x572e99abu, 0x267492abu, 0x85a763afu, 0xcb3e287eu, 0x2bc28b99u, 0x32acd2b0u, 0x2ea734ccu, 0x0606c4a0u}; return t; }
};
struct CurveBls377 {
    static constexpr int ID = ZKHIP_CURVE_BLS12_377;
    typedef Fe<Bls377Fr> Fr;
    typedef Fe<Bls377Fq> Fq;
    typedef Fe2<Bls377Fq> Fq2;       // u^2 = -5 (Bls377Fq::BETA)
    static constexpr u64 GENERATOR = 22;
    static constexpr int TWO_ADICITY = 47;
    // generators of order r on y^2 = x^3 + 1 and on the twist y^2 = x^3 + 1/u, canonical limbs as above.  Written down as
    // [UPSTREAM] ark-bls12-377 0.3.0's G1 / G2 generators; that ark uses exactly these points is NOT checked against its source
    // (they are on their curves and of order r: tests/test_bls12_377.py).  Only a setup called without explicit generators reads
    // them; proving never does, and ark's own setup draws random generators.
    static const u32* g1_gen() { static const u32 t[] = {0xb21be9efu, 0xeab9b16eu, 0xffcd394eu, 0xd5481512u, 0xbd37cb5cu, 0x188282c8u, 0xaa9d41bbu, 0x85951e2cu, 0xbf87ff54u, 0xc8fc6225u, 0xfe740a67u, 0x008848deu, 0x559c8ea6u, 0xfd82de55u, 0x34a9591au, 0xc2fe3d36u, 0x4fb82305u, 0x6d182ad4u, 0xca3e52d9u, 0xbd7fb348u, 0x30afeec4u, 0x1f674f5du, 0xc5102effu, 0x01914a69u}; return t; }
    static const u32* g2_gen() { static const u32 t[] = {0x7c005196u, 0x74e3e48fu, 0xbb535402u, 0x71889f52u, 0x57db6b9bu, 0x7ea501f5u, 0x203e5031u, 0xc565f071u, 0xa3841d01u, 0xc89630a2u, 0x71c785feu, 0x018480beu, 0x6ea16afeu, 0xb26bfefau, 0xbff76fe6u, 0x5cf89984u, 0x0799c9deu, 0xe7223eceu, 0x6651cecbu, 0x532777eeu, 0xb1b140d5u, 0x70dc5a51u, 0xe7004031u, 0x00ea6040u, 0x09fd4ddfu, 0xf0940944u, 0x6d8c7c2eu, 0xf2cf8888u, 0xf832d204u, 0xe458c282u, 0x74b49a58u, 0xde03ed72u, 0xcbb2efb4u, 0xd960736bu, 0x5d446f7bu, 0x00690d66u, 0x85eb8f93u, 0xd9a1cdd1u, 0x5e52270bu, 0x4279b83fu, 0xcee304c2u, 0x2463b01au, 0x3d591bf1u, 0x61ef11acu, 0x151a70aau, 0x9e549da3u, 0xd2835518u, 0x00f8169fu}; return t; }
};

struct ApiError {
    int32_t code;
    std::string msg;
};
static inline void require(bool ok, int32_t code, const char* msg) {
    if (!ok) throw ApiError{code, msg};
}
// what both uploads of an assignment say of a first element that is not the constant
static const char* const Z0_NOT_ONE_MSG = "z[0] must be 1 (ark instance variable 0 is the constant ONE)";

// ------------------------------------------------------------------ device buffers
struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    DBuf() {}
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { dev_free(p); }
    void swap(DBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    void release() { dev_free(p); p = nullptr; cap = 0; }
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        dev_free(p);
        p = nullptr;
        cap = 0;
        p = dev_alloc(bytes);
        cap = bytes;
    }
};
template <class T> static inline T* ptr(const DBuf& b) { return (T*)b.p; }

static inline unsigned blocks_for(u64 n, unsigned threads) { return (unsigned)((n + threads - 1) / threads); }
static inline int ilog2_floor(u64 x) { int l = 0; while (x >>= 1) ++l; return l; }
static inline int ilog2_ceil(u64 x) { int l = 0; while (((u64)1 << l) < x) ++l; return l; }

}  // namespace zk

using namespace zk;

// ------------------------------------------------------------------ context
struct NttPlanBase {
    int curve, logN;
    virtual ~NttPlanBase() {}
};
// result of one classification / digit / counting-sort pass; shared (read-only) by every base set paired with those scalars
struct MsmSort {
    DBuf dig, sorted, cnt, off, cursor, chunk_sum, grand;   // dig: the scalars' signed digits, window-major (k_msm_digits)
    DBuf pairs, ccur, tile_off;                             // the two-level placement: (key & 255, entry) pairs by coarse bin, the bins' cursors, tiles per bin
    Event ready = nullptr;   // recorded on the main stream when the pass is complete
};
// workspace and stream of one MSM: the five MSMs of a proof are independent once their scalars are sorted, and the
// fold stages are latency-bound (few, long dependent chains), so they run concurrently and fill each other's gaps
struct MsmLane {
    Stream stream = 0;        // made on first use (lane_stream): a stream is ~10 ms of queue set-up, and a process that proves once on
    bool made = false;        // one stream (the CLI: ZKHIP_TUNE_SERIAL) never needs the ~20 a resident prover keeps busy
    bool high_priority = false;
    DBuf lane_key, heavy, partial, bucket, rows, cols;
    Event done = nullptr;
};
static constexpr int ZK_NLANES = 5;   // A, B1, L (G1), B2 (G2) over z; H over h
static constexpr int ZK_NSLOTS = 4;   // most proofs in flight (zkhip_prove_g16*_batch pipelines consecutive proofs; ctx->nslots of them are used)
// everything one proof in flight owns: its scalars, NTT vectors, sort results, MSM workspaces, window sums and events
struct ProofSlot {
    DBuf scalars, zmont, va, vb, vc, ws1, ws2, zflag;   // zflag: one word, set by k_check_canonical when a host assignment is staged
    DBuf verdict;             // checked mode: u64 lowest failing row (~0: none), u64 failing rows (k_r1cs_check)
    int check_idx = -1;       // >= 0: the proof in flight is checked, and this is its index within the call (zkhip_ctx_set_checked)
    MsmSort sorts[3];         // over z (every table), over h, over z without the variables a family of tables holds at infinity (zkhip_pk::thin_mask)
    MsmLane lanes[ZK_NLANES];
    void* h_ws = nullptr;      // pinned host copy of the window sums
    size_t h_ws_cap = 0;
    Event ev[4] = {nullptr, nullptr, nullptr, nullptr};   // staged, MSMs over z issued, h ready, all done (copied out)
    Event acc_b[ZK_NLANES] = {}, acc_e[ZK_NLANES] = {};   // around each accumulation kernel
    Event ntt_b = nullptr, ntt_e = nullptr;               // around the transforms (7 for Groth16: 6 batched launches + 2; 5 for GM17)
    Event g1_go = nullptr;                                // a lone proof's G1 lanes held for the G2 accumulation (Prover::enqueue, g2_head_start)
    Event half_ready = nullptr;                           // a member of a multi-GPU proof: its half of the witness map (a or b on the coset) is in va
    int half = -1;                                        // which half this proof's head computed (-1: the whole witness map)
    bool lone = false;                                    // (enqueue_head -> enqueue_tail)
    // a split proof between its head and its tail (zkhip_prove_g16_split_begin .. _end, or the two phases of zkhip_prove_g16_multi):
    // PENDING.  The slot remembers the handles the head was enqueued with and whether the key was bound then; the tail takes these,
    // and until it is collected (or zkhip_prove_g16_split_abort) the context refuses every call that could touch them (split_refuse)
    bool split_pending = false;
    const zkhip_pk* split_pk = nullptr;
    const zkhip_r1cs* split_cs = nullptr;
    bool split_bound = false;
    bool ready = false;        // streams and events exist (slot_init)
    // the proof currently in flight in this slot
    bool busy = false;
    uint8_t r[32], s[32];
    // a proof whose assignment came as a witness file (WitnessZ): the plan's host tables — they name a missing variable and place the
    // public inputs when the ticket is collected, and are shared with the plan, so a plan freed in between costs nothing — and the
    // pinned copy of the head of z (l x 32 B) the inputs are read from.  Null for every other source
    std::shared_ptr<const WPlanTables> wit;
    void* h_inputs = nullptr;
    size_t h_inputs_cap = 0;
    std::chrono::steady_clock::time_point t_start;
};
// an assignment in the packed form of zkhip_assignment_pack, validated on the host (assignment_packed_validate): where its sections start
struct PackedZ {
    const uint8_t* bytes;
    size_t len;
    u64 tags_off, index_off, payload_off;
};
// an assignment as the bytes of a ZoKrates `witness` file whose framing the host has checked (witness_header_validate: `count`
// entries), to be ordered by the tables of `plan` on the device (wingest.cuh)
struct zkhip_wplan;
struct WitnessZ {
    const uint8_t* bytes;
    size_t len;
    u64 count;
    const zkhip_wplan* plan;
};
// zkhip_queue: the loop of Prover::run_batch — "enqueue i, finish i - (NS - 1)" — with the CALLER as the loop (zkhip_api.hip).  Ticket t
// is in flight in slot t % cap, the slot run_batch gives proof t; head .. next - 1 are in flight, so a submit finds its slot free
// because at most `cap` are.  While it is open its context is pending (`zkhip_ctx::queue`), as under a split proof.
struct zkhip_queue {
    zkhip_ctx* ctx = nullptr;
    const zkhip_pk* pk = nullptr;
    const zkhip_r1cs* cs = nullptr;
    u32 cap = 0;              // ctx->nslots at open
    u64 head = 0, next = 0;   // the oldest ticket in flight, the next ticket handed out
    bool checked = false;     // the context's checked mode at open
    bool broken = false;      // a device error: nothing is in flight any more, every remaining ticket collects with `dev_err`
    std::string dev_err;
};
struct zkhip_ctx {
    int device = 0;
    Stream stream = 0;        // main stream: staging, sort, mat-vec, NTTs (high priority: short kernels the H MSM waits for)
    Stream out_stream = 0;    // copies the window sums out once every MSM of a proof is done
    Stream ntt_stream = 0;    // the mat-vec / NTT / h-sort pipeline of a proof in flight (high priority): off the main stream, so that
                              // the next proof's staging and z-sort (what its four big MSMs wait for) do not queue behind it
    bool out_made = false, ntt_made = false;   // (both made on first use: ctx_out_stream, ctx_ntt_stream)
    Stream ws = 0;            // the stream the mat-vec / NTT helpers launch on right now (ntt_stream inside a proof, else `stream`)
    bool serial = false;      // ZKHIP_SERIAL=1: every MSM on the main stream (debugging / per-kernel timing)
    bool g2_first = true;     // the G2 lane's stream at high priority (see slot_init)
    // tunables (zkhip_ctx_tune; the environment variables ZKHIP_SERIAL, ZKHIP_MSM_C, ZKHIP_MSM_WAVES and
    // ZKHIP_NTT_SINGLE_MAX_LOG give their initial values, read ONCE when the context is created)
    MsmKnobs msm;             // the MSM's tunables and the device's compute units (msm_geom.h)
    int b_sort_mode = 0;      // the thinned list (zkhip_pk::thin_mask): 0 when a tenth of a family's bases are at infinity, 1 always, 2 never
    bool fuse_z = true;       // A, B1 and L of a proof (one sorted list) as ONE slicing / accumulation / fold launch each
    int z_gate = 1;           // which accumulations over z wait for the witness map of their proof: 0 none, 1 the G1 lanes, 2 all
    int g2_head_start = 1;    // a LONE proof over a curve whose G2 accumulation runs one wave per SIMD: its G1 lanes also wait for the end of
                              // that accumulation — 0 never, 1 over a bound key, 2 always (ZKHIP_G2_HEAD_START; Prover::enqueue)
    int split_min_log = 18;   // smallest domain (log2) whose witness map the members of a multi-GPU proof split between them (below: every
                              // member runs all of it — two transforms of 2^17 elements cost less than the exchange; ZKHIP_SPLIT_MIN_LOG)
    int ntt_single_max = 10;  // largest domain handled by one LDS-resident pass
    int ntt_max_sublog = 11;  // largest sub-transform of a pass (2^11 elements staged per sequence); domains above twice this take three passes
    int ntt_cols = 2;         // adjacent columns per workgroup of the cols pass (64-byte rows in HBM at 2)
    std::vector<Stream> idle_streams;   // made and left idle: the fillers between the pipes of a stream plan (make_pipe_streams)
    std::string pipe_plan;    // which dispatcher ("pipe") each stream of a resident prover sits on (ZKHIP_PIPES; make_pipe_streams below)
    bool pipes_made = false;
    Stream ntt_lone_stream = 0;              // the witness map of a LONE proof ("n" of the plan), where the plan gives it a pipe of its own choosing
    bool ntt_lone_made = false;
    int ntt_fuse_first = 1;   // the first butterfly round of a pass done on the elements as they are fetched (kernels_ntt.cuh ntt_first_round; ZKHIP_NTT_FUSE_FIRST=0: every round through LDS)
    int tenants = 1;          // contexts of one zkhip_multi that share this context's device (their keys are sized for a share of its memory)
    int nslots = 3;           // proofs in flight in the batch calls (<= ZK_NSLOTS; measured 2 / 3 / 4: 72.0 / 76.0 / 74.8 proofs/s)
    bool checked = false;     // zkhip_ctx_set_checked: the single-GPU prove calls test Az o Bz == Cz on the device and refuse a proof that fails
    struct Unsatisfied { u32 proof; u64 first_row, n_bad; };
    std::vector<Unsatisfied> unsat;   // the failing proofs of the last such call, in proof order (zkhip_ctx_unsatisfied)
    std::string err;
    std::string desc;
    ProofSlot slots[ZK_NSLOTS];
    ProofSlot* cur = &slots[0];   // the slot the primitives (ntt, msm, ...) and the next enqueue work in
    zkhip_queue* queue = nullptr; // the open proof queue of this context (zkhip_queue_open .. zkhip_queue_close): the context is pending
    DBuf tmp;
    DBuf wraw, wowner;        // the bytes of the witness file being ordered and the entry that owns each column (Prover::ingest_z); kept between calls
    Stream verify_stream = 0; // the pairing checks (pairing.cuh): a stream and buffers of their own, so that they may run while a proof queue is open
    bool verify_made = false;
    DBuf vfy[11];
    Stream exec_stream = 0;   // witnesses computed on the device (wexec.cuh): a stream and buffers of their own, as the pairing checks have
    bool exec_made = false;
    DBuf xstore, xargs, xverdict, xptrs, xfile, xinputs;   // the value store of a chunk, its arguments, verdict words, z pointers, files and inputs; kept between calls
    int exec_chunk = 0;       // instances per chunk of zkhip_compute_witness (ZKHIP_TUNE_EXEC_CHUNK; 0: from the store's bytes per instance, exec_chunk_default)
    bool exec_wide = false;   // ZKHIP_TUNE_EXEC_WIDE: zkhip_compute_witness takes the level-scheduled route (k_exec_level, k_exec_levels_run)
    int exec_wide_min = 0;    // ZKHIP_TUNE_EXEC_WIDE_MIN: the width at which a level gets a launch of its own (0: EXEC_WIDE_MIN_DEFAULT)
    u64 exec_last[4] = {0, 0, 0, 0};   // the last zkhip_compute_witness, as zkhip_exec_last reports it
    DBuf zpack;               // the packed bytes of the compact assignment being widened (zkhip_assignment_upload_packed, zkhip_queue_submit_packed); kept between calls
    std::vector<std::unique_ptr<NttPlanBase>> plans;
    // kernels whose dynamic-LDS limit has been raised for this context's device (the attribute is per device: a flag per
    // process would leave the second GPU of a process at the 64 KiB default)
    std::unordered_set<const void*> lds_opted;
    // a member of a zkhip_multi whose transforms are sharded (ntt_shard.h): the staging of its all-to-alls.  Consecutive exchanges
    // alternate between the two `send` sets: a member packs exchange e + 2 into the set of exchange e only after it has waited, in
    // exchange e + 1, for every peer's `packed` event of e + 1 — recorded on the peer's stream behind that peer's copies of e
    struct Shard {
        DBuf send[2], recv, out;
        Event packed[2] = {nullptr, nullptr};   // made once (shard_state)
        unsigned turn = 0;                      // exchanges entered so far: the next one packs into send[turn & 1]
        std::vector<uint8_t> host;              // a strip on its way in, a range on its way out
    } shard;
};
// ---- streams by dispatcher.  The hardware queues of a process are dealt round-robin to the chip's four compute dispatchers
// ("pipes") in the order they are made, whatever their priority, and a dispatch that still has workgroups to place holds its
// pipe: a kernel that arrives on another queue of that pipe waits until the whole of it is placed — 0.3 ms behind a 0.6 ms
// kernel of four rounds, 3 ms behind an accumulation — while a kernel on another pipe gets the first place that comes free
// (tools/pipe_probe.hip, profiles/r6s_pipe_probe.txt).  A proof's fold chains, transforms and sorts are short kernels that
// arrive while accumulations are being placed; which pipe their streams share with which accumulation used to be an accident
// of the order of first use.  The plan names the pipe (0..3, relative to one another) of every stream of a resident prover:
//   M main (staging, z sort)  N witness map + h sort  n a lone proof's witness map  O copy-out  |  per slot: Z, G, H the lanes of
//   A/B1/L, B2 and H.  A lane's fold chain stays on the stream of its accumulation (second streams for the folds — per lane type,
//   per slot, for lone proofs only — were measured and left out: profiles/r6r_fold_hop_and_stream_order_ab.txt, r6t_*, r6w_*)
// e.g. "M=3,N=3,O=3,G=0,Z=1,H=2"; a name followed by a slot number ("G1=2") overrides that slot.  All streams of
// the plan are made in one go, in pipe order (idle streams fill the gaps), the first time a proof is enqueued.
// the plan of a resident prover (ZKHIP_TUNE_PIPE_PLAN = 1): found by a local search over the pipe of every stream, scored on four workloads at
// once — dense 2^20 BN254, stdlib SHA-256 2^20, the Poseidon chain on BLS12-381 2^18, GM17 2^20 — batches AND lone proofs (tools/plan_search.py,
// profiles/r7f_*, r7h_*, validated in r7g and at the end of r7h).  What its good layouts share: the witness-map stream N (and a lone proof's, n) on a pipe that
// holds no A/B1/L lane and no H lane, only G2 lanes of later slots; slot 0's three lanes — the ones a lone proof uses — never three on one pipe.
// Against streams in order of first use: dense level in batches and a lone proof 0.25-0.3 ms sooner, stdlib SHA-256 +8-9 % proofs/s, Poseidon
// +3 %, GM17 level; no workload slower.  (Round 6's first plan — one pipe per lane TYPE, fold streams per type: "M=1,N=2,n=3,O=0,G=0,Z=1,H=2,
// g=3,z=3,h=3" — gave the dense circuit the same and cost the thin ones 5-15 %: profiles/r6t_*, r6w_*.)  Still a request, not a default: the
// sixteen streams cost a one-proof process 0.15 s.
#define ZK_PIPE_PLAN_RESIDENT "M=2,N=3,O=1,n=3,G0=0,Z0=1,H0=0,G1=3,Z1=1,H1=0,G2=3,Z2=2,H2=1"
struct PipeWant { Stream* target; bool* made; bool high; int cls; bool done; };
static inline void make_pipe_streams(zkhip_ctx* ctx) {
    if (ctx->pipes_made || ctx->pipe_plan.empty() || ctx->serial) return;
    ctx->pipes_made = true;
    auto find = [&](const std::string& key) -> int {       // "key=d" in the plan, -1 if absent
        size_t pos = 0;
        const std::string& pl = ctx->pipe_plan;
        while (pos < pl.size()) {
            size_t end = pl.find(',', pos);
            if (end == std::string::npos) end = pl.size();
            const std::string tok = pl.substr(pos, end - pos);
            const size_t eq = tok.find('=');
            if (eq != std::string::npos && tok.substr(0, eq) == key && eq + 1 < tok.size() && tok[eq + 1] >= '0' && tok[eq + 1] <= '3') return tok[eq + 1] - '0';
            pos = end + 1;
        }
        return -1;
    };
    std::vector<PipeWant> want;
    static bool dummy_made;
    int c;
    if ((c = find("M")) >= 0) { stream_sync(ctx->stream); stream_destroy(ctx->stream); ctx->stream = 0; want.push_back({&ctx->stream, &dummy_made, true, c, false}); }
    if ((c = find("N")) >= 0 && !ctx->ntt_made) want.push_back({&ctx->ntt_stream, &ctx->ntt_made, true, c, false});
    if ((c = find("n")) >= 0) want.push_back({&ctx->ntt_lone_stream, &ctx->ntt_lone_made, true, c, false});
    if ((c = find("O")) >= 0 && !ctx->out_made) want.push_back({&ctx->out_stream, &ctx->out_made, false, c, false});
    static const char names[3] = {'Z', 'G', 'H'};
    static const int lane_of[3] = {0, 3, 4};
    for (int k = 0; k < std::min(ctx->nslots, ZK_NSLOTS); ++k)
        for (int t = 0; t < 3; ++t) {
            MsmLane& lane = ctx->slots[k].lanes[lane_of[t]];
            const std::string up(1, names[t]);
            c = find(up + std::to_string(k)); if (c < 0) c = find(up);
            if (c >= 0 && !lane.made) want.push_back({&lane.stream, &lane.made, t == 1 && ctx->g2_first, c, false});
        }
    size_t left = want.size();
    for (int t = 0; left; ++t) {
        PipeWant* pick = nullptr;
        for (auto& w : want) if (!w.done && w.cls == (t & 3)) { pick = &w; break; }
        if (pick) { *pick->target = pick->high ? stream_create_high_priority() : stream_create(); *pick->made = true; pick->done = true; --left; }
        else ctx->idle_streams.push_back(stream_create_low_priority());      // (an idle queue of a priority nothing else uses)
    }
    ctx->ws = ctx->stream;
}
// streams and events of one proof slot, made the first time the slot is used
static inline void slot_init(zkhip_ctx* ctx, ProofSlot& sl) {
    if (sl.ready) return;
    for (auto& so : sl.sorts) so.ready = event_create();
    for (int k = 0; k < ZK_NLANES; ++k) {
        // lane 3 is the G2 MSM: the longest accumulation AND the longest fold tail of a proof; at high priority its
        // workgroups are dispatched first, it finishes early and its tail hides under the G1 accumulations
        sl.lanes[k].high_priority = k == 3 && ctx->g2_first;       // (the stream itself is made when a launch first needs it: lane_stream)
        sl.lanes[k].done = event_create();
        sl.acc_b[k] = event_create();
        sl.acc_e[k] = event_create();
    }
    for (auto& e : sl.ev) e = event_create();
    sl.ntt_b = event_create();
    sl.ntt_e = event_create();
    sl.g1_go = event_create();
    sl.half_ready = event_create();
    sl.ready = true;
}
// streams made when they are first needed
static inline Stream lane_stream(MsmLane& lane) {
    if (!lane.made) { lane.stream = lane.high_priority ? stream_create_high_priority() : stream_create(); lane.made = true; }
    return lane.stream;
}
static inline Stream ctx_out_stream(zkhip_ctx* ctx) {
    if (!ctx->out_made) { ctx->out_stream = stream_create(); ctx->out_made = true; }
    return ctx->out_stream;
}
static inline Stream ctx_ntt_stream(zkhip_ctx* ctx);
// the stream of a proof's witness map: the context's, or — a lone proof under a plan that names one — the lone proofs' own
static inline Stream slot_ntt_stream(zkhip_ctx* ctx, const ProofSlot& sl) {
    return (sl.lone && ctx->ntt_lone_made) ? ctx->ntt_lone_stream : ctx_ntt_stream(ctx);
}
static inline Stream ctx_ntt_stream(zkhip_ctx* ctx) {
    if (!ctx->ntt_made) { ctx->ntt_stream = stream_create_high_priority(); ctx->ntt_made = true; }
    return ctx->ntt_stream;
}
// gfx950 has 160 KiB of LDS per CU; anything above the 64 KiB default must be opted into, per kernel and per device
// the z-lane gate of the proof being enqueued (see Prover::enqueue)
static inline int z_gate(const zkhip_ctx* ctx) { return ctx->serial ? 0 : ctx->z_gate; }
static inline void lds_opt_in(zkhip_ctx* ctx, const void* kernel) {
#ifndef ZK_EMU
    if (ctx->lds_opted.count(kernel)) return;
    ZK_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ctx->lds_opted.insert(kernel);
#else
    (void)ctx; (void)kernel;
#endif
}

#include "ntt_host.cuh"
#include "msm_host.cuh"

namespace zk {

static inline int env_int(const char* name, int lo, int hi, int dflt) {
    if (const char* e = getenv(name)) { int v = atoi(e); if (v >= lo && v <= hi) return v; }
    return dflt;
}
// ------------------------------------------------------------------ per-group launchers (group.cuh; the MSM's: msm_host.cuh)
// binding a key to a constraint system (bind.cuh: the kernels; group.cuh: these launchers, instantiated for G1 only).  `x`: two
// vectors of N XYZZ points (bind_xyzz_bytes each); everything on ctx->stream.
template <class F>
size_t bind_xyzz_bytes();
template <class F>
void bind_scale(zkhip_ctx* ctx, const void* d_h_table, u64 N, u64 n_src, u32 n1, u32 n2, u32 n3, const u32* d_scal, const u32* d_konst, int nw, void* d_x);
template <class F>
void bind_fft(zkhip_ctx* ctx, void* d_x, u64 N, const u32* d_tw, int nw);
template <class F>
void bind_h_finish(zkhip_ctx* ctx, const void* d_x, u64 N, int logN, void* d_out);
template <class F>
void bind_cmul(zkhip_ctx* ctx, const void* d_x, int logN, const u32* d_row, const u32* d_val, int nw, const u32* d_minus_one, u64 nnz, void* d_prod);
template <class F>
void bind_l_finish(zkhip_ctx* ctx, const void* d_prod, const u64* d_cptr, const void* d_l_table, u64 m, const u32* d_long_cols, u64 n_long, void* d_sum, void* d_out);
// fixed-base tables / multiplications for setup (N3); also per-group code
template <class F>
void fixed_base_table(zkhip_ctx* ctx, const Aff<F>* h_pj, int nwin, DBuf& tbl);
template <class F>
void fixed_base_mul(zkhip_ctx* ctx, const DBuf& tbl, int nwin, const u32* d_scalars, u64 count, Aff<F>* d_out);
// TEST ONLY (zkhip_group_op, include/zkhip.h): one group-law function of ec.cuh / bind.cuh / kernels_msm.cuh element by element, in
// the form a kernel of the product calls it (bind.cuh k_group_op: one instantiation per op).  The ids are the header's.
enum GroupOp : int {
    GOP_MADD_ACC = 0, GOP_MADD_COLD, GOP_MADD_HOT, GOP_ADD_ACC, GOP_ADD_FROM, GOP_ADD, GOP_ADD_TO, GOP_DBL, GOP_DBL_INL, GOP_DBL_ACC, GOP_DBL_AFFINE,
    GOP_DBL_AFFINE_HOT, GOP_NEG_U, GOP_TO_AFFINE, GOP_TO_AFFINE_U, GOP_MUL_WORDS, GOP_MUL_U32, GOP_MUL_SMALL, GOP_MADD_ACC_NEG, GOP_ADD_FROM_NEG, GOP_COUNT
};
constexpr int GROUP_OP_SCALAR_WORDS = 8;      // words of `k` per element
// which ops exist for (group, form): the saturated form has what the fixed-base kernels and the host run; the unsaturated form what the
// MSM, fold and bind kernels run — the bind kernels over G1 only (they alone subtract: xyzz_add_from with neg), and nothing there uses
// the exact-zero tests of xyzz_add.  `neg` is a constant of the instantiation, as it is at every call in the product: a kernel that took
// it at run time changed how the units' shared out-of-line routines were compiled, and with them the frames of the fold kernels.
constexpr bool group_op_known(int group, int form, int op) {
    if (group < 1 || group > 2 || form < 0 || form > 1 || op < 0 || op >= GOP_COUNT) return false;
    const bool sat_only = op == GOP_ADD || op == GOP_ADD_TO || op == GOP_MUL_U32 || op == GOP_TO_AFFINE;
    if (form == 0) return sat_only || op == GOP_MADD_ACC || op == GOP_DBL;      // (GOP_MADD_ACC_NEG, GOP_ADD_FROM_NEG: form 1)
    if (sat_only) return false;
    if (group == 2 && (op == GOP_NEG_U || op == GOP_TO_AFFINE_U || op == GOP_MUL_WORDS || op == GOP_ADD_FROM_NEG)) return false;
    return true;
}
// FS: the group's saturated coordinate field (Fq or Fq2); a, b, out: count x 4 coordinates of raw limbs in the form's layout
template <class FS>
void group_op_run(zkhip_ctx* ctx, int form, int op, u64 count, const u32* a, const u32* b, const u32* k, const uint8_t* flags, u32* out);

// ------------------------------------------------------------------ byte codecs (host)
template <class F>
static F fe_from_bytes_canon(const uint8_t* b) {   // canonical LE bytes -> canonical limbs (no Montgomery)
    F x;
    memcpy(x.v, b, F::BYTES);
    return x;
}
template <class P>
static bool canon_lt_mod(const Fe<P>& x) {
    for (int i = P::N - 1; i >= 0; --i) {
        if (x.v[i] != P::mod(i)) return x.v[i] < P::mod(i);
    }
    return false;
}
// ark uncompressed affine -> canonical coords with infinity as all-zero (the device sentinel)
template <int FQ_BYTES, int NCOORD>
static void decode_point(const uint8_t* src, uint8_t* dst) {
    constexpr int SZ = FQ_BYTES * NCOORD;
    const bool inf = src[SZ - 1] & 0x40;
    if (inf) { memset(dst, 0, SZ); return; }
    memcpy(dst, src, SZ);
    dst[SZ - 1] &= 0x3f;
}
template <class F> static void write_fe(const F& mont, uint8_t* out) { F c = fe_from_mont(mont); memcpy(out, c.v, F::BYTES); }

}  // namespace zk

// ------------------------------------------------------------------ proving key
struct zkhip_pk {
    int curve;
    int scheme = 0;                               // 0 = Groth16, 1 = GM17 (gm17.cuh: same five MSM lanes, other bases)
    zkhip_ctx* ctx;
    u64 m, w, l, hlen, N;
    int logN;
    DBuf a_ext, b1_ext, l_ext, b2_ext, h_sigma;   // Montgomery affine, MSM-ready
    std::vector<uint8_t> delta_g1_canon;          // for the -rs*delta_1 term of C (host)
    std::vector<uint8_t> g_gamma2_z2_canon;       // GM17: for the rho^2 * g_gamma2_z2 term of C (host)
    // Multi-GPU sharding of ONE proof (zkhip_pk_load_g16_shard): this key holds the bases of the index ranges
    // [z_lo, z_lo + z_n) of the extended variable range [0, m+2) and [h_lo, h_lo + h_n) of the sigma-ordered h range
    // [0, N); every rank derives the same window widths from the nominal (largest) range length.
    u32 rank = 0, world = 1;
    u64 z_lo = 0, z_n = 0, h_lo = 0, h_n = 0;
    int c_z = 0, c_h = 0;
    // The thinned list.  Variables that do not occur in the B matrix have the point at infinity in b_g1_query AND b_g2_query (a
    // third of the Poseidon chain's); a GM17 key holds it for the same half of its variables in a_query, c_query_2 and b_query.
    // The z tables that hold many such bases (a tenth or more) form a family (`thin_mask`: bit k = table k of a_ext, b1_ext,
    // l_ext, b2_ext) whose MSMs pair with a sorted list of their own that leaves out the variables at infinity in ALL of them
    // (`thin_keep`: one bit per entry of the z range, set where some base of the family is finite) — one more counting sort, and
    // the most expensive MSMs of a real circuit shrink by that share.  0: every table on the common list.
    DBuf thin_keep;
    u32 thin_mask = 0;
    bool inf_many_thin[4] = {true, true, true, true};   // inf_many of the family's tables on the thinned list
    bool inf_many[5] = {true, true, true, true, true};   // per table (a, b1, l, b2, h): more than one base in 2048 is the point at
                                                       // infinity -> the accumulation lets lanes sit those out (MsmShape::skip_inf)
    int s_z = 1, s_h = 1;     // bucket sets of the MSMs over z / over h = every s-th window multiple is in the tables (MsmShape::sets)
    // log2 N1 of the NTT plan the sigma order of h_sigma was made for (N = N1 * N2): a context whose plan for this domain
    // splits differently (ZKHIP_TUNE_NTT_SINGLE_MAX_LOG changed after the key was loaded, or an image written under
    // another setting) would pair h with the wrong bases, so the provers and zkhip_pk_import refuse the mismatch
    int ntt_log1 = -1;
    // Bound to one constraint system (zkhip_pk_bind_r1cs, PkLoader::bind): H' = the coset inverse transform applied to h_query
    // (natural order: it pairs with the quotient's EVALUATIONS on the coset), L' = l_query with c's share of the quotient folded in
    // per variable.  Proofs over the system `bound_uid` names take four transforms and two mat-vecs (a GM17 key: two transforms); any
    // other system takes the tables above.  A shard holds its index ranges of H' and L' (zkhip_pk_bind_r1cs_shard).  0 = not bound.
    DBuf h_bound, l_bound;
    u64 bound_uid = 0;
    u64 bound_fp[2] = {0, 0};                // fingerprint of that system (PkLoader::r1cs_fingerprint): what a key image remembers of it — a key
                                             // imported with its bound tables is attached by zkhip_pk_bind_r1cs when the fingerprints agree,
                                             // without recomputing anything
    bool inf_many_bound[2] = {true, true};   // (L', H'): as inf_many
};

// Device-layout image of a loaded key (zkhip_pk_export / _import; PkLoader<C>::export_image / import_image).  "ZKHIPPK" + layout
// version; bump the version whenever the resident layout (packed points, sigma order, the extended base vectors, table levels)
// changes: an image is only meaningful to the library build that wrote it.  An image holds level 0 of the five base tables; the
// window multiples are recomputed on the device at import (~0.1 s for a 2^20 key — less than reading the 6 GiB they occupy from any
// disk: measured in round 3, which is why the image that carried every level is gone).
static const char PK_IMAGE_MAGIC[8] = {'Z', 'K', 'H', 'I', 'P', 'P', 'K', '5'};
struct PkImageHeader {
    char magic[8];
    int32_t curve, scheme;
    uint64_t m, w, l, hlen, N;
    int32_t logN, c_z, c_h, sets;     // sets: s_z | s_h << 8 — which window multiples the tables hold (MsmShape::sets)
    uint32_t rank, world;
    int32_t ntt_split, reserved;      // the NTT split h_sigma is ordered for (zkhip_pk::ntt_log1 = NttPlan::split())
    uint64_t z_lo, z_n, h_lo, h_n;
    uint64_t len_delta, len_g2z2, len_buf[5];
    // version 5: level 0 of the bound tables H' / L' (this key's index ranges) when the key was bound at export, and the fingerprint
    // of the constraint system they were made for — zkhip_pk_bind_r1cs on the imported key attaches them when the system's
    // fingerprint agrees and costs a checksum instead of the transforms (0 / 0: the key was not bound)
    uint64_t len_bound[2];            // H', L'
    uint64_t bound_fp[2];
};

// every constraint system of a process has a number of its own (a key remembers WHICH system it was bound to: an address can be
// handed out again after zkhip_r1cs_free)
static inline u64 zk_next_uid() {
    static std::atomic<u64> next{1};
    return next.fetch_add(1);
}
struct zkhip_r1cs {
    u64 uid = zk_next_uid();
    int curve;
    zkhip_ctx* ctx;
    u64 n, l, w, N;
    int logN;
    DBuf rp[3], col[3], val[3];
    u64 nnz[3];
    u64 nnz_short[3];     // without the rows of more than MATVEC_LONG terms (what the lanes-per-row choice of k_matvec is made from)
    DBuf long_rows;       // those rows, matrix << 32 | row (k_matvec_long); the first n_huge of them have more than MATVEC_HUGE terms (k_matvec_huge)
    u64 n_long = 0, n_huge = 0;
    u64 fp[2] = {0, 0};   // PkLoader::r1cs_fingerprint, computed when first asked for
    bool fp_made = false;
};
// lanes per row of k_matvec for a launch over the matrices [mat0, mat0 + nmat) (a matrix outside the launch counts as 1):
// what Prover::matvec launches with and what zkhip_r1cs_matvec_shape reports
static inline void matvec_lanes(const zkhip_r1cs* cs, int g[3], int nmat = 3, int mat0 = 0) {
    for (int k = 0; k < 3; ++k) g[k] = (k >= mat0 && k < mat0 + nmat) ? matvec_group(cs->nnz_short[k], cs->n) : 1;
}
// the matrices of a resident constraint system back in host memory (setup, N3: key generation walks them on the host; the
// prover never needs them there, so zkhip_r1cs_load keeps no host copy).  Values come back as they are resident:
// saturated Montgomery form.
struct HostCsr {
    std::vector<u64> rp[3];
    std::vector<u32> col[3];
    std::vector<uint8_t> val[3];
    void fetch(zkhip_ctx* ctx, const zkhip_r1cs* cs) {
        for (int k = 0; k < 3; ++k) {
            rp[k].resize(cs->n + 1);
            col[k].resize(cs->nnz[k]);
            val[k].resize(cs->nnz[k] * 32);
            dev_d2h(rp[k].data(), cs->rp[k].p, (cs->n + 1) * 8, ctx->stream);
            if (cs->nnz[k]) {
                dev_d2h(col[k].data(), cs->col[k].p, cs->nnz[k] * 4, ctx->stream);
                dev_d2h(val[k].data(), cs->val[k].p, cs->nnz[k] * 32, ctx->stream);
            }
        }
        stream_sync(ctx->stream);
    }
};

// an assignment resident in HBM: (m + 2) x 32 B canonical integers; the two tail slots receive r and s
struct zkhip_assignment {
    int curve;
    zkhip_ctx* ctx;
    u64 m;
    DBuf scalars;
};

// zkhip_wplan: the column order of one program, resident — the two id -> column tables of wplan.h on the device, what the host needs
// of them (shared with the proof slots that hold a proof made through the plan), and which system it was made for
struct zkhip_wplan {
    zkhip_ctx* ctx = nullptr;
    u64 cs_uid = 0;
    std::shared_ptr<const WPlanTables> host;
    DBuf pos, neg;
};

// zkhip_xplan: the statements of one program compiled for k_exec_program (xplan.h), resident: the instruction stream, the
// coefficients, the entries of a witness file and the public-input slots on the device, and the host's copy.  (What it has of the
// constraint system it was made from — l, w, the columns — is in the host's copy: nothing of the system is read again.)
struct zkhip_xplan {
    zkhip_ctx* ctx = nullptr;
    std::shared_ptr<const XPlanHost> host;
    DBuf code, pool, file_ids, file_slots, input_cols;
    DBuf sched, level_start;      // the level schedule (xplan.h: xplan_schedule), for the level-scheduled route
};
// The width at and above which a level of the schedule is a launch of k_exec_level of its own; narrower levels share a launch of
// k_exec_levels_run with their neighbours.  The sweep over 64 .. 8192 at one instance was flat on the program measured (DESIGN §3 "A
// lone witness across the device", profiles/device_exec_wide.json), so it fixes nothing: 1024 is four strides of the run kernel's
// workgroup, inside the 256 .. 4096 that were defensible beforehand, and keeps a program of narrower levels at the fewest launches.
static constexpr int EXEC_WIDE_MIN_DEFAULT = 1024;
static constexpr int EXEC_WIDE_MIN_MAX = 1 << 20;
static inline Stream ctx_exec_stream(zkhip_ctx* ctx) {
    if (!ctx->exec_made) { ctx->exec_stream = stream_create(); ctx->exec_made = true; }
    return ctx->exec_stream;
}
// Instances per chunk when the caller names none.  `bytes_per_instance`: everything the call keeps per instance of a chunk — the value
// store (slots x 32 B: 32 MiB for a program of 2^20 variables), the arguments, and the file and the inputs where they are asked for.  The
// kernel wants as many waves as the device has room for: half of the device memory that is free or already held by this context's
// exec buffers (so that a second call finds the chunk of the first), 32 GiB at most, in whole waves (one wave at least, 65536
// instances at most).  The other half is left to the assignments the call delivers, which are the caller's to budget.
static inline u64 exec_chunk_default(const zkhip_ctx* ctx, u64 bytes_per_instance) {
    size_t free_b = 0, total_b = 0;
    dev_mem_info(&free_b, &total_b);
    const u64 held = ctx->xstore.cap + ctx->xargs.cap + ctx->xverdict.cap + ctx->xptrs.cap + ctx->xfile.cap + ctx->xinputs.cap;
    const u64 budget = std::min<u64>(((u64)free_b + held) / 2, (u64)32 << 30);
    const u64 fit = budget / std::max<u64>(bytes_per_instance, 32);
    return std::min<u64>(std::max<u64>(fit / WX_BLOCK * WX_BLOCK, WX_BLOCK), 65536);
}

namespace zk {

// ------------------------------------------------------------------ the window sums of a proof slot
// What the five lanes of a proof over `pk` leave, and where: `G1 ws1[4][Wmax]` (A, B1, L over z; H over h) and `G2 ws2[Wmax]` (B2) on
// the device, and the slot's pinned record on the host — a mirror of both (every lane copies its own sums out), the word of the
// canonical check behind them and, 8 bytes on, the 16-byte verdict of checked mode.  The only place that knows this layout.
template <class C>
struct SlotSums {
    typedef Xyzz<typename C::Fq> G1;
    typedef Xyzz<typename C::Fq2> G2;
    MsmShape shz, shh;   // the MSMs over z / over h
    int Wmax;            // sums per MSM (2: the tables carry the window multiples)
    // (a sharded key covers only its index range of the bases; the shapes are recomputed from the key's own (c, sets): a key whose
    // numbers this build cannot run is refused, never paired with a sort of another window width)
    SlotSums(const zkhip_ctx* ctx, const zkhip_pk* pk)
        : shz(msm_shape(&ctx->msm,pk->z_n, C::Fr::Params::BITS, true, pk->c_z, pk->s_z)), shh(msm_shape(&ctx->msm,pk->h_n, C::Fr::Params::BITS, true, pk->c_h, pk->s_h)) {
        require(shz.c == pk->c_z && shh.c == pk->c_h && (int)shz.sets == pk->s_z && (int)shh.sets == pk->s_h, ZKHIP_ERR_BAD_ARG,
                "the key's tables were built for a window width this build cannot sort: reload the key");
        Wmax = (int)std::max(shz.nsums(), shh.nsums());
    }
    size_t b1() const { return (size_t)4 * Wmax * sizeof(G1); }
    size_t b2() const { return (size_t)Wmax * sizeof(G2); }
    size_t lane_bytes() const { return (size_t)Wmax * sizeof(G1); }
    size_t record_bytes() const { return b1() + b2() + 24; }
    template <class T> T* lane(T* g1_sums, int k) const { return g1_sums + (size_t)k * Wmax; }   // MSM k of 4 x Wmax G1 sums, wherever they are
    G1* ws1(const ProofSlot& sl, int k) const { return lane(ptr<G1>(sl.ws1), k); }
    G2* ws2(const ProofSlot& sl) const { return ptr<G2>(sl.ws2); }
    G1* hs1(const ProofSlot& sl, int k) const { return lane((G1*)sl.h_ws, k); }
    G2* hs2(const ProofSlot& sl) const { return (G2*)((uint8_t*)sl.h_ws + b1()); }
    uint8_t* zflag(const ProofSlot& sl) const { return (uint8_t*)sl.h_ws + b1() + b2(); }
    uint8_t* verdict(const ProofSlot& sl) const { return zflag(sl) + 8; }
    u32 zflag_word(const ProofSlot& sl) const { u32 f; memcpy(&f, zflag(sl), 4); return f; }
    // the slot's buffers, large enough for this key
    void reserve(ProofSlot& sl) const {
        sl.ws1.ensure(b1());
        sl.ws2.ensure(b2());
        if (sl.h_ws_cap < record_bytes()) {
            host_free_pinned(sl.h_ws);
            sl.h_ws = nullptr; sl.h_ws_cap = 0;
            sl.h_ws = host_alloc_pinned(record_bytes());
            sl.h_ws_cap = record_bytes();
        }
    }
};

// What a proving-key file of either scheme says a key is (PkLoader::parse_g16 / parse_gm17; pointers into the file's bytes, ark's
// canonical encoding): four base tables over the extended variable range [0, m + 2), each a query vector at a shift, one extra point
// at one index and optionally a constant folded into entry 0, in the resident order a, b1, l, b2 (b2: G2); the bases of the quotient
// with their count before the padding; and the points the host formula for C needs.
struct KeySources {
    int scheme;                       // 0 = Groth16, 1 = GM17
    u64 m, w, l, hlen, N;             // as zkhip_pk
    struct Lane {
        const uint8_t* src; u64 nsrc, shift;       // entry shift + j = src[j], j < nsrc
        const uint8_t* extra; u64 extra_at;        // entry extra_at = *extra (if any); every other entry: the point at infinity
        const uint8_t* add0;                       // added to entry 0 (if any)
    } lane[4];
    const uint8_t* h_src; u64 h_nsrc;
    const uint8_t *delta_g1, *g_gamma2_z2;         // Groth16 / GM17: null in a key of the other scheme
};
// the square arithmetic program a GM17 key is made for (gm17.cuh): M variables, D0 rows padded to the radix-2 domain D
struct SapShape {
    u64 M, D0, D;
    int logD;
};
static inline SapShape sap_shape(u64 n, u64 l, u64 w) {
    SapShape s;
    s.M = 1 + 2 * (l - 1) + w + n;
    s.D0 = 2 * n + 2 * (l - 1) + 1;
    s.logD = ilog2_ceil(s.D0);
    s.D = (u64)1 << s.logD;
    return s;
}

template <class C>
struct PkLoader {
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    static constexpr int FQB = Fq::BYTES;
    static constexpr int G1B = 2 * FQB, G2B = 4 * FQB;

    struct Rd {
        const uint8_t* p;
        const uint8_t* e;
        const uint8_t* take(size_t n) {
            require((size_t)(e - p) >= n, ZKHIP_ERR_PARSE, "proving key truncated");
            const uint8_t* r = p;
            p += n;
            return r;
        }
        u64 len(size_t elem) {
            u64 n;
            memcpy(&n, take(8), 8);
            require(n <= (u64)(e - p) / elem, ZKHIP_ERR_PARSE, "proving key vector length exceeds file size");
            return n;
        }
    };

    // `count` points of NC base-field coordinates each, resident in Montgomery form: entry shift + j is ark's encoding src[j]
    // (j < nsrc), entry `extra_at` the single point `extra` (if any), every other entry the point at infinity.  Decoded straight
    // into the pinned staging ring on a few host threads (dev_h2d_fill): one pass through host memory.
    template <int NC>
    static void upload_decoded(zkhip_ctx* ctx, DBuf& dst, u64 count, const uint8_t* src, u64 nsrc, u64 shift, const uint8_t* extra, u64 extra_at) {
        constexpr size_t PB = (size_t)FQB * NC;
        dst.ensure(count * PB);
        dev_h2d_fill(dst.p, count * PB, PB, ctx->stream, [=](char* out, size_t off, size_t len) {
            const u64 i0 = off / PB, i1 = (off + len) / PB;
            for (u64 i = i0; i < i1; ++i) {
                uint8_t* o = (uint8_t*)out + (i - i0) * PB;
                if (i >= shift && i - shift < nsrc) decode_point<FQB, NC>(src + (i - shift) * PB, o);
                else if (extra && i == extra_at) decode_point<FQB, NC>(extra, o);
                else memset(o, 0, PB);
            }
        });
        ZK_LAUNCH((k_to_mont<Fq>), dim3(blocks_for(count * NC, 256)), dim3(256), 0, ctx->stream, ptr<Fq>(dst), ptr<Fq>(dst), count * NC);
        stream_sync(ctx->stream);
    }
    // dev[idx] += P (host round trip of one point; P canonical ark encoding)
    template <class F, int NC>
    static void add_into(zkhip_ctx* ctx, DBuf& buf, u64 idx, const uint8_t* ark_point) {
        uint8_t dec[G2B];
        decode_point<FQB, NC>(ark_point, dec);
        Aff<F> add;
        memcpy(&add, dec, sizeof(add));
        add = to_mont_point(add);
        Aff<F> cur;
        dev_d2h(&cur, ptr<Aff<F>>(buf) + idx, sizeof(cur), ctx->stream);
        stream_sync(ctx->stream);
        Aff<F> sum = xyzz_to_affine(xyzz_madd(Xyzz<F>::from_affine(cur), add));
        dev_h2d(ptr<Aff<F>>(buf) + idx, &sum, sizeof(sum), ctx->stream);
        stream_sync(ctx->stream);
    }
    static Aff<Fq> to_mont_point(const Aff<Fq>& p) { return {fe_to_mont(p.x), fe_to_mont(p.y)}; }
    static Aff<Fq2> to_mont_point(const Aff<Fq2>& p) { return {fe_to_mont(p.x), fe_to_mont(p.y)}; }

    static void range_of(u64 total, u32 rank, u32 world, u64& lo, u64& n, u64& nominal) {
        nominal = (total + world - 1) / world;
        lo = std::min<u64>((u64)rank * nominal, total);
        n = std::min<u64>(nominal, total - lo);
    }
    // ark's `serialize_unchecked` of ark_groth16::ProvingKey: vk{alpha_g1, beta_g2, gamma_g2, delta_g2,
    // gamma_abc_g1[]}, beta_g1, delta_g1, a_query[], b_g1_query[], b_g2_query[] (G2), h_query[], l_query[].  The tables are extended by
    // the (delta, r) and (delta, s) pairs — see prove() — and z_0 = 1, so alpha / beta ride on entry 0 of their query vectors:
    //   lane 0  A_ext  = [a_query..., delta_1, inf]       + alpha_1      lane 2  L_ext  = [inf x l, l_query..., inf, inf]
    //   lane 1  B1_ext = [b_g1_query..., inf, delta_1]    + beta_1       lane 3  B2_ext = [b_g2_query..., inf, delta_2]   + beta_2
    static KeySources parse_g16(const uint8_t* bytes, size_t len) {
        Rd rd{bytes, bytes + len};
        KeySources k{};
        k.scheme = 0;
        const uint8_t* alpha_g1 = rd.take(G1B);
        const uint8_t* beta_g2 = rd.take(G2B);
        rd.take(G2B);                                  // gamma_g2 (verifier only)
        const uint8_t* delta_g2 = rd.take(G2B);
        const u64 n_abc = rd.len(G1B);
        rd.take(n_abc * G1B);                          // gamma_abc_g1 (verifier only)
        const uint8_t* beta_g1 = rd.take(G1B);
        k.delta_g1 = rd.take(G1B);
        k.m = rd.len(G1B);
        const uint8_t* a_q = rd.take(k.m * G1B);
        const u64 mb1 = rd.len(G1B);
        const uint8_t* b1_q = rd.take(mb1 * G1B);
        const u64 mb2 = rd.len(G2B);
        const uint8_t* b2_q = rd.take(mb2 * G2B);
        k.hlen = k.h_nsrc = rd.len(G1B);
        k.h_src = rd.take(k.hlen * G1B);
        k.w = rd.len(G1B);
        const uint8_t* l_q = rd.take(k.w * G1B);
        require(rd.p == rd.e, ZKHIP_ERR_PARSE, "trailing bytes after proving key");
        require(k.m >= 1 && mb1 == k.m && mb2 == k.m && k.w <= k.m, ZKHIP_ERR_PARSE, "inconsistent query lengths in proving key");
        k.l = k.m - k.w;
        require(n_abc == k.l, ZKHIP_ERR_PARSE, "gamma_abc length != number of instance variables");
        k.N = k.hlen + 1;
        require((k.N & (k.N - 1)) == 0, ZKHIP_ERR_PARSE, "h_query length + 1 is not a power of two");
        require(k.m + 2 < ((u64)1 << 31), ZKHIP_ERR_BAD_ARG, "too many variables");
        k.lane[0] = {a_q, k.m, 0, k.delta_g1, k.m, alpha_g1};
        k.lane[1] = {b1_q, k.m, 0, k.delta_g1, k.m + 1, beta_g1};
        k.lane[2] = {l_q, k.w, k.l, nullptr, 0, nullptr};
        k.lane[3] = {b2_q, k.m, 0, delta_g2, k.m + 1, beta_g2};
        return k;
    }
    // ark's `serialize_unchecked` of ark_gm17::ProvingKey: vk{h_g2, g_alpha_g1, h_beta_g2, g_gamma_g1, h_gamma_g2, query[]}, a_query[],
    // b_query[] (G2), c_query_1[], c_query_2[], g_gamma_z, h_gamma_z (G2), g_ab_gamma_z, g_gamma2_z2, g_gamma2_z_t[].  The same five
    // lanes with other bases (gm17.cuh has the algebra), extended by the (., rho) pair and one unused slot:
    //   lane 0  [a_query, g_gamma_z, inf]                       lane 2  [inf x l, c_query_1, g_ab_gamma_z, inf]
    //   lane 1  [c_query_2, inf, inf]                           lane 3  [b_query, h_gamma_z, inf]
    // and over h g_gamma2_z_t[0 .. D) (entry D pairs with the d1^2 coefficient of ark's h, which the restructured prover does not produce)
    static KeySources parse_gm17(const uint8_t* bytes, size_t len) {
        Rd rd{bytes, bytes + len};
        KeySources k{};
        k.scheme = 1;
        rd.take(G2B); rd.take(G1B); rd.take(G2B); rd.take(G1B); rd.take(G2B);   // vk points (verifier only)
        k.l = rd.len(G1B);
        rd.take(k.l * G1B);                                                      // vk.query (verifier only)
        const u64 M = k.m = rd.len(G1B);
        const uint8_t* a_q = rd.take(M * G1B);
        const u64 Mb = rd.len(G2B);
        const uint8_t* b_q = rd.take(Mb * G2B);
        k.w = rd.len(G1B);
        const uint8_t* c1_q = rd.take(k.w * G1B);
        const u64 Mc2 = rd.len(G1B);
        const uint8_t* c2_q = rd.take(Mc2 * G1B);
        const uint8_t* g_gamma_z = rd.take(G1B);
        const uint8_t* h_gamma_z = rd.take(G2B);
        const uint8_t* g_ab_gamma_z = rd.take(G1B);
        k.g_gamma2_z2 = rd.take(G1B);
        k.hlen = rd.len(G1B);
        k.h_src = rd.take(k.hlen * G1B);
        require(rd.p == rd.e, ZKHIP_ERR_PARSE, "trailing bytes after proving key");
        require(k.l >= 1 && M >= k.l && Mb == M && Mc2 == M && k.w == M - k.l, ZKHIP_ERR_PARSE, "inconsistent query lengths in GM17 proving key");
        require(k.hlen >= 2 && ((k.hlen - 1) & (k.hlen - 2)) == 0, ZKHIP_ERR_PARSE, "g_gamma2_z_t length - 1 is not a power of two");
        require(M + 2 < ((u64)1 << 31), ZKHIP_ERR_BAD_ARG, "too many variables");
        k.N = k.h_nsrc = k.hlen - 1;
        k.lane[0] = {a_q, M, 0, g_gamma_z, M, nullptr};
        k.lane[1] = {c2_q, M, 0, nullptr, 0, nullptr};
        k.lane[2] = {c1_q, k.w, k.l, g_ab_gamma_z, M, nullptr};
        k.lane[3] = {b_q, M, 0, h_gamma_z, M, nullptr};
        return k;
    }
    // THE list of a key's five resident tables, the four lanes over z and h: fn(k, buffer, Tag<field of the coordinates>, first index and
    // count of this key's range [, the shape of the MSM the table serves: over z or over h])
    template <class F> struct Tag { typedef F type; static constexpr int NC = std::is_same<F, Fq2>::value ? 4 : 2; };   // NC: base-field coordinates per point
    template <class Fn>
    static void for_each_table(zkhip_pk* pk, Fn&& fn) {
        fn(0, pk->a_ext, Tag<Fq>{}, pk->z_lo, pk->z_n);
        fn(1, pk->b1_ext, Tag<Fq>{}, pk->z_lo, pk->z_n);
        fn(2, pk->l_ext, Tag<Fq>{}, pk->z_lo, pk->z_n);
        fn(3, pk->b2_ext, Tag<Fq2>{}, pk->z_lo, pk->z_n);
        fn(4, pk->h_sigma, Tag<Fq>{}, pk->h_lo, pk->h_n);
    }
    template <class Fn>
    static void for_each_table(zkhip_pk* pk, const MsmShape& shz, const MsmShape& shh, Fn&& fn) {
        for_each_table(pk, [&](int k, DBuf& b, auto f, u64 lo, u64 n) { fn(k, b, f, lo, n, &b == &pk->h_sigma ? shh : shz); });
    }
    static KeySources parse(int scheme, const uint8_t* bytes, size_t len) { return scheme == 0 ? parse_g16(bytes, len) : parse_gm17(bytes, len); }
    template <int NC>
    static void upload_lane(zkhip_ctx* ctx, DBuf& dst, u64 count, const KeySources::Lane& q) {
        upload_decoded<NC>(ctx, dst, count, q.src, q.nsrc, q.shift, q.extra, q.extra_at);
    }
    // the h source in file order (affine), and from there in the sigma order the plan's NTT pipeline leaves h in, padded with infinity
    static void upload_h(zkhip_ctx* ctx, const KeySources& k, DBuf& h_nat) {
        upload_decoded<2>(ctx, h_nat, std::max<u64>(k.h_nsrc, 1), k.h_src, k.h_nsrc, 0, nullptr, 0);
    }
    static void sigma_order(zkhip_ctx* ctx, NttPlan<C>* plan, const KeySources& k, const DBuf& h_nat, DBuf& h_sigma) {
        h_sigma.ensure(k.N * G1B);
        ZK_LAUNCH((k_sigma_gather_points<Aff<Fq>>), dim3(blocks_for(k.N, 256)), dim3(256), 0, ctx->stream, ptr<Aff<Fq>>(h_nat), ptr<Aff<Fq>>(h_sigma), k.N, k.h_nsrc,
                  plan->N1, plan->N2, plan->N3);
    }
    static void set_dims(zkhip_pk* pk, const KeySources& k) {
        pk->scheme = k.scheme;
        pk->m = k.m; pk->w = k.w; pk->l = k.l; pk->hlen = k.hlen; pk->N = k.N; pk->logN = ilog2_floor(k.N);
    }
    // a parsed key of either scheme, resident: the four lanes over z, the h table, the constants on entry 0, the window multiples
    static void load(zkhip_ctx* ctx, const KeySources& k, zkhip_pk* pk) {
        set_dims(pk, k);
        NttPlan<C>* plan = get_plan<C>(ctx, pk->logN);
        pk->ntt_log1 = plan->split();
        if (k.delta_g1) pk->delta_g1_canon.assign(k.delta_g1, k.delta_g1 + G1B);
        if (k.g_gamma2_z2) pk->g_gamma2_z2_canon.assign(k.g_gamma2_z2, k.g_gamma2_z2 + G1B);
        const u64 me = k.m + 2;
        for_each_table(pk, [&](int j, DBuf& b, auto f, u64, u64) {
            if (j < 4) upload_lane<decltype(f)::NC>(ctx, b, me, k.lane[j]);
        });
        {
            DBuf h_nat;
            upload_h(ctx, k, h_nat);
            sigma_order(ctx, plan, k, h_nat, pk->h_sigma);
            stream_sync(ctx->stream);
        }
        for_each_table(pk, [&](int j, DBuf& b, auto f, u64, u64) {
            if (j < 4 && k.lane[j].add0) add_into<typename decltype(f)::type, decltype(f)::NC>(ctx, b, 0, k.lane[j].add0);
        });
        finish_tables(ctx, pk, me, k.N);
    }
    static void load_file(zkhip_ctx* ctx, int scheme, const uint8_t* bytes, size_t len, zkhip_pk* pk) { load(ctx, parse(scheme, bytes, len), pk); }

    template <class F> static u64 table_bytes(u64 count, u32 levels) { return std::max<u64>(count, 1) * (u64)levels * packed_point_bytes<F>(); }
    // bytes the five tables take at these shapes (an empty table still holds one point per level: what to_table allocates)
    static u64 tables_need(zkhip_pk* pk, const MsmShape& shz, const MsmShape& shh) {
        u64 t = 0;
        for_each_table(pk, shz, shh, [&](int, DBuf&, auto f, u64, u64 n, const MsmShape& sh) { t += table_bytes<typename decltype(f)::type>(n, sh.levels); });
        return t;
    }
    // this rank's share of the bases (everything for world = 1) as MSM tables: level 0 = the packed working form of the
    // range's points, levels 1 .. W-1 their window multiples 2^(c j) P (a 2^20 BN254 key: 16 levels, 6 GiB of the 288)
    static void finish_tables(zkhip_ctx* ctx, zkhip_pk* pk, u64 me, u64 hdom) {
        u64 nominal_z, nominal_h;
        range_of(me, pk->rank, pk->world, pk->z_lo, pk->z_n, nominal_z);
        range_of(hdom, pk->rank, pk->world, pk->h_lo, pk->h_n, nominal_h);
        auto shape_z = [&](int sets) { return msm_shape(&ctx->msm,nominal_z, C::Fr::Params::BITS, true, 0, sets); };
        auto shape_h = [&](int sets) { return msm_shape(&ctx->msm,nominal_h, C::Fr::Params::BITS, true, 0, sets); };
        // Every window multiple of every base (one bucket set, one fold per MSM) while that fits the device: a 2^20 key is 6 GiB,
        // 2^24 96 GiB.  Beyond — or when ZKHIP_TUNE_MSM_SETS says so — the tables keep every 2nd, 4th, ... multiple and the MSMs
        // fold as many bucket sets (the reference has no size limit below the field's two-adicity; this is how it is met).
        // (one count for both, doubled until it has passed the windows of the MSMs over z: one bucket set per window there)
        int sets = ctx->msm.msm_sets;
        if (!sets) {
            const MsmShape one = shape_z(0);
            const u64 budget = msm_table_budget(ctx, pk->z_n, pk->h_n, hdom, one.W, one.K);
            const int no_cap = 1 << 30;
            sets = msm_pick_sets({1, 1}, {no_cap, no_cap}, {one.W + 1, 0}, budget, [&](MsmSets s) { return tables_need(pk, shape_z(s.z), shape_h(s.h)); }).z;
        }
        const MsmShape shz = shape_z(sets), shh = shape_h(sets);
        pk->c_z = shz.c;
        pk->c_h = shh.c;
        pk->s_z = (int)shz.sets;
        pk->s_h = (int)shh.sets;
        for_each_table(pk, shz, shh, [&](int, DBuf& b, auto f, u64 lo, u64 n, const MsmShape& sh) { to_table<typename decltype(f)::type>(ctx, b, lo, n, sh); });
        count_points_at_infinity(ctx, pk);
    }
    // levels 1 .. W-1 of the five tables of a key whose level 0 is in place (import of a compact image)
    static void table_levels(zkhip_ctx* ctx, zkhip_pk* pk) {
        const SlotSums<C> ly(ctx, pk);
        for_each_table(pk, ly.shz, ly.shh, [&](int, DBuf& b, auto f, u64, u64 n, const MsmShape& sh) {
            msm_table_levels<typename decltype(f)::type>(ctx, b.p, n, sh.level_bits(), (int)sh.levels);
        });
        count_points_at_infinity(ctx, pk);
    }
    // ---- zkhip_pk_bind_r1cs: H' and L' for ONE constraint system (bind.cuh has the algebra) ----
    static void unbind(zkhip_pk* pk) {
        pk->bound_uid = 0;
        pk->bound_fp[0] = pk->bound_fp[1] = 0;
        pk->h_bound.release();
        pk->l_bound.release();
    }
    // position-keyed checksum of a resident constraint system (dimensions, the three matrices as they are resident): cached
    static void r1cs_fingerprint(zkhip_ctx* ctx, const zkhip_r1cs* cs_, u64 fp[2]) {
        zkhip_r1cs* cs = const_cast<zkhip_r1cs*>(cs_);
        if (!cs->fp_made) {
            DBuf d;
            d.ensure(16);
            Stream s = ctx->stream;
            dev_memset(d.p, 0, 16, s);
            for (int k = 0; k < 3; ++k) {
                const u64 salt = 0xA5A5A5A5ull * (u64)(k + 1) + cs->n * 0x9E3779B97F4A7C15ull + cs->l * 0xC2B2AE3D27D4EB4Full + cs->w;
                auto run = [&](const void* p, u64 bytes, u64 tag) {
                    if (bytes) ZK_LAUNCH(k_fingerprint, dim3(1024), dim3(256), 0, s, (const u32*)p, bytes / 4, salt ^ (tag * 0x165667B19E3779F9ull), (unsigned long long*)d.p);
                };
                run(cs->rp[k].p, (cs->n + 1) * 8, 1);
                run(cs->col[k].p, cs->nnz[k] * 4, 2);
                run(cs->val[k].p, cs->nnz[k] * 32, 3);
            }
            dev_d2h(cs->fp, d.p, 16, s);
            stream_sync(s);
            cs->fp[0] ^= (u64)cs->curve + 1;           // (never all zero for an empty system either)
            cs->fp_made = true;
        }
        fp[0] = cs->fp[0];
        fp[1] = cs->fp[1];
    }
    // the quotient's domain, the bases it pairs with and the variable range of either scheme
    struct BindShape {
        u64 N, n_src, me, mcols;    // domain; h bases that are not the padding; entries of the l table; variables (columns of W)
        int logN;
    };
    static BindShape bind_shape(const zkhip_pk* pk) {
        BindShape b;
        b.N = pk->N; b.logN = pk->logN; b.mcols = pk->m; b.me = pk->m + 2;
        b.n_src = pk->scheme == 0 ? pk->hlen : pk->N;     // Groth16: h_query has N - 1 entries; GM17: g_gamma2_z_t[0 .. D)
        return b;
    }
    // THE test that a key belongs to a constraint system: curve, scheme (`want_scheme`: what the caller is about to run), dimensions
    // (`min_N`: the smallest domain the caller can use)
    static void check_match(const zkhip_pk* pk, const zkhip_r1cs* cs, int want_scheme, u64 min_N = 1) {
        require(pk->curve == C::ID && cs->curve == C::ID, ZKHIP_ERR_BAD_ARG, "curve mismatch between key and constraint system");
        require(pk->scheme == want_scheme, ZKHIP_ERR_BAD_ARG,
                want_scheme == 0 ? "this is a GM17 proving key: use zkhip_prove_gm17" : "this is a Groth16 proving key: use zkhip_prove_g16");
        if (pk->scheme == 0) {
            require(pk->m == cs->l + cs->w && pk->w == cs->w && pk->N == cs->N, ZKHIP_ERR_BAD_ARG,
                    "proving key does not match the constraint system (m, w or domain size)");
        } else {
            const SapShape sh = sap_shape(cs->n, cs->l, cs->w);
            require(pk->m == sh.M && pk->l == cs->l && pk->N == sh.D && pk->N >= min_N, ZKHIP_ERR_BAD_ARG,
                    "GM17 proving key does not match the constraint system (SAP variables, instance size or domain)");
        }
    }
    // everything a refusal can depend on, BEFORE anything of the key is touched (zkhip_pk_bind_r1cs)
    static void bind_check(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs) {
        check_match(pk, cs, pk->scheme, 2);
        if (pk->scheme == 0) require(pk->N >= 2 && pk->hlen + 1 == pk->N, ZKHIP_ERR_BAD_ARG, "domain too small to bind");
        NttPlan<C>* pl = get_plan<C>(ctx, pk->logN);
        require(pl->split() == pk->ntt_log1, ZKHIP_ERR_BAD_ARG, "the key's h bases were ordered for another NTT split (NTT_SINGLE_MAX_LOG changed): reload the key");
    }
    // W — the matrix whose product with the assignment the quotient subtracts (Groth16: C; GM17: the SAP's) — by COLUMNS, on the
    // host: crow[cptr[v] .. cptr[v+1]) = the rows variable v occurs in, cval the coefficients (saturated Montgomery form, as the
    // matrices are resident), long_cols the variables with more than BIND_SHORT_COL entries
    struct WCols {
        std::vector<u64> cptr;
        std::vector<u32> crow, long_cols;
        std::vector<uint8_t> cval;
        u64 nnz() const { return crow.size(); }
    };
    // `extra[v]`: entries variable v gets besides C's (GM17); each C entry lands on row row_mul * k with its value times val_mul4 ? 4 : 1
    struct WExtra { u32 col, row; int four; };
    static void w_columns(zkhip_ctx* ctx, const zkhip_r1cs* cs, u64 mcols, u32 row_mul, bool val_mul4, const std::vector<WExtra>& extra, WCols& W) {
        typedef typename C::Fr Fr;
        static_assert(sizeof(Fr) == 32 && Fr::N <= 12, "the binding's scalar routines take up to 12 words; Fr is 32 bytes on both curves");
        Stream s = ctx->stream;
        const u64 nnz = cs->nnz[2];
        std::vector<u64> rp(cs->n + 1);
        std::vector<u32> col(nnz);
        std::vector<uint8_t> val(nnz * sizeof(Fr));
        dev_d2h(rp.data(), cs->rp[2].p, (cs->n + 1) * 8, s);
        if (nnz) {
            dev_d2h(col.data(), cs->col[2].p, nnz * 4, s);
            dev_d2h(val.data(), cs->val[2].p, nnz * sizeof(Fr), s);
        }
        stream_sync(s);
        W.cptr.assign(mcols + 1, 0);
        for (u64 e = 0; e < nnz; ++e) {
            require(col[e] < mcols, ZKHIP_ERR_BAD_ARG, "internal: column index out of range");
            ++W.cptr[col[e] + 1];
        }
        for (const WExtra& x : extra) ++W.cptr[x.col + 1];
        for (u64 v = 0; v < mcols; ++v) W.cptr[v + 1] += W.cptr[v];
        const u64 total = W.cptr[mcols];
        W.crow.resize(total);
        W.cval.resize(total * sizeof(Fr));
        std::vector<u64> cur(W.cptr.begin(), W.cptr.end() - 1);
        for (u64 k = 0; k < cs->n; ++k)
            for (u64 e = rp[k]; e < rp[k + 1]; ++e) {
                const u64 at = cur[col[e]]++;
                W.crow[at] = (u32)(k * row_mul);
                Fr v;
                memcpy(v.v, &val[e * sizeof(Fr)], sizeof(Fr));
                if (val_mul4) v = fe_dbl(fe_dbl(v));
                memcpy(&W.cval[at * sizeof(Fr)], v.v, sizeof(Fr));
            }
        const Fr one = Fr::one(), four = fe_dbl(fe_dbl(Fr::one()));
        for (const WExtra& x : extra) {
            const u64 at = cur[x.col]++;
            W.crow[at] = x.row;
            memcpy(&W.cval[at * sizeof(Fr)], (x.four ? four : one).v, sizeof(Fr));
        }
        W.long_cols.clear();
        for (u64 v = 0; v < mcols; ++v)
            if (W.cptr[v + 1] - W.cptr[v] > BIND_SHORT_COL) W.long_cols.push_back((u32)v);
    }
    // Level 0 of H' (N points, NATURAL order) and of L' (me points) from level 0 of the key's h table (sigma order, N entries, packed)
    // and of its padded l table (me entries, packed), both covering the WHOLE index range, on this context's device.
    static void bind_level0(zkhip_ctx* ctx, NttPlan<C>* pl, const BindShape& b, const void* d_h0, const void* d_l0, const WCols& W, DBuf& h_out, DBuf& l_out) {
        typedef typename C::Fr Fr;
        constexpr int NW = Fr::N;
        const u64 N = b.N, nnz = W.nnz();
        const u64 g1 = packed_point_bytes<Fq>(), xb = bind_xyzz_bytes<Fq>();
        {   // the transforms' points and W's products are transient, like the levels' workspace
            size_t free_b = 0, total_b = 0;
            dev_mem_info(&free_b, &total_b);
            const u64 need = (N + b.me) * g1 + 2 * N * xb + nnz * (xb + 4 + 32) + b.mcols * (xb + 8) + N * 48 + ((u64)1 << 30);
            require(need < free_b, ZKHIP_ERR_NOMEM, "not enough device memory to bind the key (the transforms' workspace)");
        }
        Stream s = ctx->stream;
        const unsigned T = 256;
        // canonical-integer scalars: g^-i / N (what the bases of H' are scaled by), w^-e (the transform's roots), -1 / (N Z(g)), p - 1
        DBuf d_scal, d_tw, d_k;
        d_scal.ensure(N * sizeof(Fr));
        d_tw.ensure(std::max<u64>(N / 2, 1) * sizeof(Fr));
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(N, T)), dim3(T), 0, s, ptr<Fr>(d_scal), pl->g_inv, pl->n_inv, N, 0u, 0u, 0, 1u);
        ZK_LAUNCH((k_from_mont<Fr>), dim3(blocks_for(N, T)), dim3(T), 0, s, ptr<Fr>(d_scal), ptr<Fr>(d_scal), N);
        ZK_LAUNCH((k_pow_table<Fr>), dim3(blocks_for(N / 2, T)), dim3(T), 0, s, ptr<Fr>(d_tw), pl->omega_inv, Fr::one(), N / 2, 0u, 0u, 0, 1u);
        ZK_LAUNCH((k_from_mont<Fr>), dim3(blocks_for(N / 2, T)), dim3(T), 0, s, ptr<Fr>(d_tw), ptr<Fr>(d_tw), N / 2);
        Fr konst[2];
        konst[0] = fe_from_mont(fe_neg(fe_mul(pl->n_inv, pl->zinv)));
        konst[1] = fe_from_mont(fe_neg(Fr::one()));
        d_k.ensure(sizeof(konst));
        dev_h2d(d_k.p, konst, sizeof(konst), s);
        stream_sync(s);                                // (konst is on this frame)
        // the two transforms over the bases: vector 0 -> H' (coset), vector 1 -> H'' (what W's columns are summed against)
        DBuf x;
        x.ensure(2 * N * xb);
        bind_scale<Fq>(ctx, d_h0, N, b.n_src, pl->N1, pl->N2, pl->N3, ptr<u32>(d_scal), ptr<u32>(d_k), NW, x.p);
        bind_fft<Fq>(ctx, x.p, N, ptr<u32>(d_tw), NW);
        h_out.ensure(N * g1);
        bind_h_finish<Fq>(ctx, x.p, N, b.logN, h_out.p);
        stream_sync(s);
        d_scal.release();
        d_tw.release();
        // W by columns: D_v = sum_k W[k][v] H''_k, added to the l base of v
        DBuf d_cptr, d_crow, d_cval, d_long, prod, sum;
        d_cptr.ensure((b.mcols + 1) * 8);
        d_crow.ensure(std::max<u64>(nnz, 1) * 4);
        d_cval.ensure(std::max<u64>(nnz, 1) * 32);
        d_long.ensure(std::max<u64>(W.long_cols.size(), 1) * 4);
        prod.ensure(std::max<u64>(nnz, 1) * xb);
        sum.ensure(std::max<u64>(b.mcols, 1) * xb);
        dev_h2d(d_cptr.p, W.cptr.data(), (b.mcols + 1) * 8, s);
        if (!W.long_cols.empty()) dev_h2d(d_long.p, W.long_cols.data(), W.long_cols.size() * 4, s);
        if (nnz) {
            dev_h2d(d_crow.p, W.crow.data(), nnz * 4, s);
            dev_h2d(d_cval.p, W.cval.data(), nnz * 32, s);
            ZK_LAUNCH((k_from_mont<Fr>), dim3(blocks_for(nnz, T)), dim3(T), 0, s, ptr<Fr>(d_cval), ptr<Fr>(d_cval), nnz);   // resident values: Montgomery form
            bind_cmul<Fq>(ctx, (const uint8_t*)x.p + N * xb, b.logN, ptr<u32>(d_crow), ptr<u32>(d_cval), NW, ptr<u32>(d_k) + NW, nnz, prod.p);
        }
        l_out.ensure(b.me * g1);
        dev_d2d((uint8_t*)l_out.p + b.mcols * g1, (const uint8_t*)d_l0 + b.mcols * g1, (b.me - b.mcols) * g1, s);   // the slots behind the variables: as in l's table
        bind_l_finish<Fq>(ctx, prod.p, ptr<u64>(d_cptr), d_l0, b.mcols, ptr<u32>(d_long), W.long_cols.size(), sum.p, l_out.p);
        stream_sync(s);                                // (the host vectors were the copies' sources)
    }
    // this key's index ranges of H' / L' as MSM tables (level 0 from `h_src` / `l_src`: this key's RANGES, h_n / z_n points, on the
    // host or — `on_device` — on this device), the window multiples behind them, the counts the accumulation kernel is chosen from
    static void install_bound(zkhip_ctx* ctx, zkhip_pk* pk, const void* h_src, const void* l_src, bool on_device, const u64 fp[2]) {
        const SlotSums<C> ly(ctx, pk);
        const MsmShape &shz = ly.shz, &shh = ly.shh;
        const u64 g1 = packed_point_bytes<Fq>();
        {
            size_t free_b = 0, total_b = 0;
            dev_mem_info(&free_b, &total_b);
            const u64 need = pk->h_n * shh.levels * g1 + pk->z_n * shz.levels * g1 + ((u64)2 << 30);
            require(need < free_b, ZKHIP_ERR_NOMEM, "not enough device memory to bind the key (two more MSM tables)");
        }
        Stream s = ctx->stream;
        pk->h_bound.ensure(std::max<u64>(pk->h_n, 1) * (u64)shh.levels * g1);
        pk->l_bound.ensure(std::max<u64>(pk->z_n, 1) * (u64)shz.levels * g1);
        auto put = [&](DBuf& dst, const void* src, u64 bytes) {
            if (!bytes) return;
            if (on_device) dev_d2d(dst.p, src, bytes, s);
            else dev_h2d_fill(dst.p, bytes, 64, s, [src](char* out, size_t off, size_t len) { memcpy(out, (const char*)src + off, len); });
        };
        put(pk->h_bound, h_src, pk->h_n * g1);
        put(pk->l_bound, l_src, pk->z_n * g1);
        stream_sync(s);
        msm_table_levels<Fq>(ctx, pk->h_bound.p, pk->h_n, shh.level_bits(), (int)shh.levels);
        msm_table_levels<Fq>(ctx, pk->l_bound.p, pk->z_n, shz.level_bits(), (int)shz.levels);
        pk->inf_many_bound[0] = count_infinite<Fq>(ctx, pk->l_bound.p, pk->z_n) * 2048 > pk->z_n;
        pk->inf_many_bound[1] = count_infinite<Fq>(ctx, pk->h_bound.p, pk->h_n) * 2048 > pk->h_n;
        pk->bound_fp[0] = fp[0];
        pk->bound_fp[1] = fp[1];
    }
    static void w_columns_for(zkhip_ctx* ctx, int scheme, const zkhip_r1cs* cs, u64 mcols, WCols& W) {
        if (scheme == 0) { w_columns(ctx, cs, mcols, 1, false, {}, W); return; }
        // GM17: W = the SAP's right-hand sides (gm17.cuh: rows 2k: 4 C_k + e_k, 2k+1: e_k, 2n: 1, 2n+2i-1: 4 x_i + f_i, 2n+2i: f_i)
        const u64 n = cs->n, l = cs->l, m = cs->l + cs->w;
        std::vector<WExtra> extra;
        extra.reserve(2 * n + 3 * l);
        extra.push_back({0u, (u32)(2 * n), 0});
        for (u64 i = 1; i < l; ++i) extra.push_back({(u32)i, (u32)(2 * n + 2 * i - 1), 1});
        for (u64 k = 0; k < n; ++k) { extra.push_back({(u32)(m + k), (u32)(2 * k), 0}); extra.push_back({(u32)(m + k), (u32)(2 * k + 1), 0}); }
        for (u64 i = 1; i < l; ++i) { extra.push_back({(u32)(m + n - 1 + i), (u32)(2 * n + 2 * i - 1), 0}); extra.push_back({(u32)(m + n - 1 + i), (u32)(2 * n + 2 * i), 0}); }
        w_columns(ctx, cs, mcols, 2, true, extra, W);
    }
    // zkhip_pk_bind_r1cs on a key that covers the whole index range (or one whose imported bound tables only need attaching)
    static void bind(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* cs) {
        bind_check(ctx, pk, cs);
        u64 fp[2];
        r1cs_fingerprint(ctx, cs, fp);
        if (pk->h_bound.p && pk->l_bound.p && pk->bound_fp[0] == fp[0] && pk->bound_fp[1] == fp[1] && (fp[0] | fp[1])) {
            pk->bound_uid = cs->uid;                    // the tables are there already (an imported image, or the same system loaded again)
            return;
        }
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG,
                "a shard of a multi-GPU key binds through zkhip_pk_bind_r1cs_shard / zkhip_multi_bind (the transforms need every base of the key once)");
        unbind(pk);
        NttPlan<C>* pl = get_plan<C>(ctx, pk->logN);
        const BindShape b = bind_shape(pk);
        require(pk->z_n == b.me && pk->h_n == b.N, ZKHIP_ERR_BAD_ARG, "internal: an unsharded key covers the whole index range");
        WCols W;
        w_columns_for(ctx, pk->scheme, cs, b.mcols, W);
        DBuf h0, l0;
        bind_level0(ctx, pl, b, pk->h_sigma.p, pk->l_ext.p, W, h0, l0);
        install_bound(ctx, pk, h0.p, l0.p, true, fp);
        pk->bound_uid = cs->uid;
    }
    // Level 0 of H' and L' over the WHOLE index range, from the key FILE (a shard holds only its ranges of the bases; the transforms
    // need all of them once), left in host memory: every member of a multi-GPU prover then installs its own ranges
    // (zkhip_multi_bind: one member computes, all install; zkhip_pk_bind_r1cs_shard: a rank of a multi-process prover does both).
    static void bound_level0_from_file(zkhip_ctx* ctx, int scheme, const zkhip_r1cs* cs, const uint8_t* bytes, size_t len, std::vector<uint8_t>& h_host,
                                       std::vector<uint8_t>& l_host, u64 fp[2]) {
        const KeySources k = parse(scheme, bytes, len);
        zkhip_pk tmp;                                   // dimensions and level 0 of the two tables only
        tmp.curve = C::ID; tmp.ctx = ctx;
        set_dims(&tmp, k);
        DBuf l_aff, h_nat, h_sig;
        upload_lane<2>(ctx, l_aff, k.m + 2, k.lane[2]);
        upload_h(ctx, k, h_nat);
        NttPlan<C>* pl = get_plan<C>(ctx, tmp.logN);
        tmp.ntt_log1 = pl->split();
        bind_check(ctx, &tmp, cs);
        const BindShape b = bind_shape(&tmp);
        const u64 g1 = packed_point_bytes<Fq>();
        DBuf h0p, l0p;
        sigma_order(ctx, pl, k, h_nat, h_sig);
        h0p.ensure(b.N * g1);
        l0p.ensure(b.me * g1);
        points_to_packed<Fq>(ctx, ptr<Aff<Fq>>(h_sig), h0p.p, b.N);
        points_to_packed<Fq>(ctx, ptr<Aff<Fq>>(l_aff), l0p.p, b.me);
        stream_sync(ctx->stream);
        h_nat.release(); l_aff.release(); h_sig.release();
        WCols W;
        w_columns_for(ctx, scheme, cs, b.mcols, W);
        DBuf h0, l0;
        bind_level0(ctx, pl, b, h0p.p, l0p.p, W, h0, l0);
        h_host.resize(b.N * g1);
        l_host.resize(b.me * g1);
        dev_d2h(h_host.data(), h0.p, h_host.size(), ctx->stream);
        dev_d2h(l_host.data(), l0.p, l_host.size(), ctx->stream);
        stream_sync(ctx->stream);
        r1cs_fingerprint(ctx, cs, fp);
    }
    // a member's share of a binding computed elsewhere: its ranges of the whole-range level-0 arrays
    static void install_bound_ranges(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* h_full, size_t h_len, const uint8_t* l_full, size_t l_len,
                                     const u64 fp[2]) {
        bind_check(ctx, pk, cs);
        const BindShape b = bind_shape(pk);
        const u64 g1 = packed_point_bytes<Fq>();
        require(h_len == b.N * g1 && l_len == b.me * g1, ZKHIP_ERR_BAD_ARG, "internal: bound level-0 arrays of another key");
        u64 have[2];
        r1cs_fingerprint(ctx, cs, have);
        require(have[0] == fp[0] && have[1] == fp[1], ZKHIP_ERR_BAD_ARG, "internal: the binding was computed for another constraint system");
        unbind(pk);
        install_bound(ctx, pk, h_full + pk->h_lo * g1, l_full + pk->z_lo * g1, false, fp);
        pk->bound_uid = cs->uid;
    }
    // ---- device-layout image of a loaded key (PkImageHeader): level 0 of the five tables, and of H' / L' if the key was bound ----
    static u64 export_size(const zkhip_pk* pk_) {
        zkhip_pk* pk = const_cast<zkhip_pk*>(pk_);
        u64 t = sizeof(PkImageHeader) + pk->delta_g1_canon.size() + pk->g_gamma2_z2_canon.size();
        for_each_table(pk, [&](int, DBuf&, auto f, u64, u64 n) { t += table_bytes<typename decltype(f)::type>(n, 1); });
        if (pk->h_bound.p && pk->l_bound.p) t += table_bytes<Fq>(pk->h_n, 1) + table_bytes<Fq>(pk->z_n, 1);
        return t;
    }
    static void export_image(zkhip_pk* pk, uint8_t* out, u64 cap) {
        zkhip_ctx* ctx = pk->ctx;
        require(cap >= export_size(pk), ZKHIP_ERR_BAD_ARG, "output buffer too small (see zkhip_pk_export_size)");
        PkImageHeader h;
        memset(&h, 0, sizeof(h));
        memcpy(h.magic, PK_IMAGE_MAGIC, 8);
        h.curve = pk->curve; h.scheme = pk->scheme;
        h.m = pk->m; h.w = pk->w; h.l = pk->l; h.hlen = pk->hlen; h.N = pk->N;
        h.logN = pk->logN; h.c_z = pk->c_z; h.c_h = pk->c_h; h.sets = pk->s_z | (pk->s_h << 8);
        h.rank = pk->rank; h.world = pk->world;
        h.ntt_split = pk->ntt_log1;
        h.z_lo = pk->z_lo; h.z_n = pk->z_n; h.h_lo = pk->h_lo; h.h_n = pk->h_n;
        h.len_delta = pk->delta_g1_canon.size(); h.len_g2z2 = pk->g_gamma2_z2_canon.size();
        const bool with_bound = pk->h_bound.p && pk->l_bound.p;
        if (with_bound) {
            h.len_bound[0] = table_bytes<Fq>(pk->h_n, 1);
            h.len_bound[1] = table_bytes<Fq>(pk->z_n, 1);
            h.bound_fp[0] = pk->bound_fp[0]; h.bound_fp[1] = pk->bound_fp[1];
        }
        uint8_t* p = out + sizeof(h);
        memcpy(p, pk->delta_g1_canon.data(), h.len_delta); p += h.len_delta;
        memcpy(p, pk->g_gamma2_z2_canon.data(), h.len_g2z2); p += h.len_g2z2;
        for_each_table(pk, [&](int k, DBuf& b, auto f, u64, u64 n) {
            h.len_buf[k] = table_bytes<typename decltype(f)::type>(n, 1);
            dev_d2h(p, b.p, h.len_buf[k], ctx->stream);     // level 0 leads every table
            p += h.len_buf[k];
        });
        memcpy(out, &h, sizeof(h));
        if (with_bound) {
            dev_d2h(p, pk->h_bound.p, h.len_bound[0], ctx->stream); p += h.len_bound[0];
            dev_d2h(p, pk->l_bound.p, h.len_bound[1], ctx->stream); p += h.len_bound[1];
        }
        stream_sync(ctx->stream);
    }
    // `pk`: a fresh key of this curve and context; the caller has checked the length against the header's size, the magic and the curve id
    static void import_image(zkhip_ctx* ctx, const uint8_t* bytes, size_t len, zkhip_pk* pk) {
        PkImageHeader h;
        memcpy(&h, bytes, sizeof(h));
        require(h.scheme == 0 || h.scheme == 1, ZKHIP_ERR_PARSE, "key image: unknown scheme");
        u64 total = sizeof(PkImageHeader), rest = len - sizeof(PkImageHeader);
        const u64 parts[9] = {h.len_delta, h.len_g2z2, h.len_buf[0], h.len_buf[1], h.len_buf[2], h.len_buf[3], h.len_buf[4], h.len_bound[0], h.len_bound[1]};
        for (u64 part : parts) {
            require(part <= rest, ZKHIP_ERR_PARSE, "key image truncated");
            rest -= part;
            total += part;
        }
        require(total == len, ZKHIP_ERR_PARSE, "trailing bytes after key image");
        int s_z = h.sets & 0xff, s_h = (h.sets >> 8) & 0xff;
        require(h.world >= 1 && h.rank < h.world && h.logN >= 0 && h.logN <= 3 * NTT_MAX_SUBLOG && h.N == ((u64)1 << h.logN) && h.z_n <= h.m + 2 &&
                    h.h_n <= h.N && h.c_z >= 2 && h.c_z <= MSM_MAX_C && h.c_h >= 2 && h.c_h <= MSM_MAX_C && s_z >= 1 && s_h >= 1 && (h.sets >> 16) == 0,
                ZKHIP_ERR_PARSE, "key image: inconsistent header");
        pk->scheme = h.scheme;
        pk->m = h.m; pk->w = h.w; pk->l = h.l; pk->hlen = h.hlen; pk->N = h.N; pk->logN = h.logN;
        pk->c_z = h.c_z; pk->c_h = h.c_h; pk->rank = h.rank; pk->world = h.world;
        pk->z_lo = h.z_lo; pk->z_n = h.z_n; pk->h_lo = h.h_lo; pk->h_n = h.h_n;
        pk->ntt_log1 = h.ntt_split;
        auto shape_z = [&](int sets) { return msm_shape(&ctx->msm,h.z_n, C::Fr::Params::BITS, true, h.c_z, sets); };
        auto shape_h = [&](int sets) { return msm_shape(&ctx->msm,h.h_n, C::Fr::Params::BITS, true, h.c_h, sets); };
        // the index ranges must lie inside the key and the five base arrays must have exactly the size the ranges imply:
        // the kernels trust these numbers
        bool sizes_ok = h.m + 2 < ((u64)1 << 31) && h.z_lo <= h.m + 2 && h.z_n <= h.m + 2 - h.z_lo && h.h_lo <= h.N && h.h_n <= h.N - h.h_lo &&
                        h.len_delta <= 4096 && h.len_g2z2 <= 4096;
        for_each_table(pk, [&](int k, DBuf&, auto f, u64, u64 n) {
            sizes_ok = sizes_ok && h.len_buf[k] == table_bytes<typename decltype(f)::type>(n, 1);
        });
        const bool with_bound = h.len_bound[0] || h.len_bound[1];
        if (with_bound)
            sizes_ok = sizes_ok && h.len_bound[0] == table_bytes<Fq>(h.h_n, 1) && h.len_bound[1] == table_bytes<Fq>(h.z_n, 1) && (h.bound_fp[0] | h.bound_fp[1]) != 0;
        require(sizes_ok, ZKHIP_ERR_PARSE, "key image: array sizes do not match the header");
        require(get_plan<C>(ctx, h.logN)->split() == h.ntt_split, ZKHIP_ERR_PARSE,
                "key image: written under another NTT split (NTT_SINGLE_MAX_LOG / NTT_MAX_SUBLOG) than this context uses; re-import the proving key");
        // The image carries level 0 only and the window multiples are recomputed here, so how many of them THIS device keeps is this
        // context's decision, not the exporter's: ZKHIP_TUNE_MSM_SETS if set, else the header's count, doubled until the tables fit
        // the budget of finish_tables (an image written on an empty 288 GB device must still load beside other tenants, with more
        // bucket sets instead of an allocation failure) — each MSM clamped to its own number of windows
        {
            const int W_z = shape_z(1).W, W_h = shape_h(1).W;
            const int fixed = ctx->msm.msm_sets;
            const u64 budget = msm_table_budget(ctx, h.z_n, h.h_n, h.N, W_z, shape_z(1).K);
            if (fixed) s_z = std::min(fixed, W_z), s_h = std::min(fixed, W_h);
            else {
                const MsmSets s = msm_pick_sets({s_z, s_h}, {W_z, W_h}, {W_z, W_h}, budget, [&](MsmSets t) { return tables_need(pk, shape_z(t.z), shape_h(t.h)); });
                s_z = s.z, s_h = s.h;
            }
        }
        // (c, sets) must be a shape this context's sort can run
        const MsmShape shz = shape_z(s_z), shh = shape_h(s_h);
        require(shz.c == h.c_z && (int)shz.sets == s_z && shh.c == h.c_h && (int)shh.sets == s_h, ZKHIP_ERR_PARSE,
                "key image: window width / bucket sets not usable under this context's settings; re-import the proving key");
        pk->s_z = s_z; pk->s_h = s_h;
        const uint8_t* p = bytes + sizeof(h);
        pk->delta_g1_canon.assign(p, p + h.len_delta); p += h.len_delta;
        pk->g_gamma2_z2_canon.assign(p, p + h.len_g2z2); p += h.len_g2z2;
        for_each_table(pk, shz, shh, [&](int k, DBuf& b, auto f, u64, u64 n, const MsmShape& sh) {
            b.ensure(table_bytes<typename decltype(f)::type>(n, sh.levels));
            const uint8_t* src = p;
            dev_h2d_fill(b.p, h.len_buf[k], 64, ctx->stream, [src](char* out, size_t off, size_t len) { memcpy(out, src + off, len); });
            p += h.len_buf[k];
        });
        stream_sync(ctx->stream);
        table_levels(ctx, pk);                     // recompute the window multiples behind level 0
        // ... and behind level 0 of H' / L'; attached to a system by zkhip_pk_bind_r1cs (fingerprint)
        if (with_bound) install_bound(ctx, pk, p, p + h.len_bound[0], false, h.bound_fp);
    }
    static void count_points_at_infinity(zkhip_ctx* ctx, zkhip_pk* pk) {
        u64 cnt[5];
        for_each_table(pk, [&](int k, DBuf& b, auto f, u64, u64 n) {
            cnt[k] = count_infinite<typename decltype(f)::type>(ctx, b.p, n);
            pk->inf_many[k] = cnt[k] * 2048 > n;
        });
        // the thinned list (zkhip_pk::thin_mask): ZKHIP_TUNE_B_SORT 0 = the tables a tenth of whose bases are at infinity, if leaving
        // out what they share drops a tenth of the list; 1 = the families the key formats predict, whatever the counts; 2 = never
        const bool gm17 = pk->scheme == 1;
        u32 family = 0;
        if (ctx->b_sort_mode == 1) family = gm17 ? 0xbu : 0xau;          // GM17: a, c_query_2, b; Groth16: b_g1, b_g2
        else if (ctx->b_sort_mode == 0)
            for (int k = 0; k < 4; ++k)
                if (cnt[k] * 10 > pk->z_n) family |= 1u << k;
        pk->thin_mask = 0;
        pk->thin_keep.release();
        if (family && pk->z_n) {
            const size_t words = (size_t)((pk->z_n + 31) / 32);
            pk->thin_keep.ensure(words * 4);
            dev_memset(pk->thin_keep.p, 0, words * 4, ctx->stream);
            for_each_table(pk, [&](int k, DBuf& b, auto f, u64, u64 n) {
                if (family >> k & 1) mark_finite<typename decltype(f)::type>(ctx, b.p, n, ptr<u32>(pk->thin_keep));      // (bits 0 .. 3: the tables over z)
            });
            std::vector<u32> host(words);
            dev_d2h(host.data(), pk->thin_keep.p, words * 4, ctx->stream);
            stream_sync(ctx->stream);
            u64 left_out = 0;
            for (u64 i = 0; i < pk->z_n; ++i) left_out += !((host[i >> 5] >> (i & 31)) & 1u);
            if (ctx->b_sort_mode == 1 || left_out * 10 > pk->z_n) {
                pk->thin_mask = family;
                // what the family's tables still meet at infinity on the thinned list
                for (int k = 0; k < 4; ++k) pk->inf_many_thin[k] = (cnt[k] - std::min(cnt[k], left_out)) * 2048 > pk->z_n;
            } else {
                pk->thin_keep.release();          // (the tables' points at infinity do not coincide: nothing to gain)
            }
        }
    }
    template <class F>
    static void to_table(zkhip_ctx* ctx, DBuf& buf, u64 lo, u64 count, const MsmShape& sh) {
        DBuf out;
        out.ensure(table_bytes<F>(count, sh.levels));
        if (count) points_to_packed<F>(ctx, ptr<Aff<F>>(buf) + lo, out.p, count);
        stream_sync(ctx->stream);
        buf.swap(out);
        out.release();                        // the saturated copy goes before the levels' workspace is allocated
        msm_table_levels<F>(ctx, buf.p, count, sh.level_bits(), (int)sh.levels);
    }
};

// ------------------------------------------------------------------ prover
template <class C>
struct Prover {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef SlotSums<C> Lay;
    typedef Transforms<C> Tr;
    static constexpr int FQB = Fq::BYTES;

    static CsrDev csr(const zkhip_r1cs* cs, int k) { return CsrDev{ptr<u64>(cs->rp[k]), ptr<u32>(cs->col[k]), cs->val[k].p}; }

    // K1: a = A z, b = B z, c = C z over rows [0, n) (+ the l instance rows of A), zero-filled up to N
    // (`nmat` = 2: A and B only — a key bound to the system carries c's share in its bases; the long rows of C, if any, still
    // land in the c vector, which nothing reads then)
    // (`mat0`: the first matrix of the launch — a member of a multi-GPU proof that transforms b only runs mat0 = 1, nmat = 1)
    static void matvec(zkhip_ctx* ctx, const zkhip_r1cs* cs, const Fr* zmont, Fr* a, Fr* b, Fr* c, u64 n, u64 l, u64 N, int nmat = 3, int mat0 = 0) {
        int g[3];
        matvec_lanes(cs, g, nmat, mat0);
        ZK_LAUNCH((k_matvec<Fr>), dim3(blocks_for(N, 256 / gmax_rows(g)), nmat), dim3(256), 0, ctx->ws, csr(cs, 0), csr(cs, 1), csr(cs, 2), zmont, a, b, c, n,
                  l, N, g[0], g[1], g[2], cs->l + cs->w, mat0);
        if (cs->n_huge)
            ZK_LAUNCH((k_matvec_huge<Fr>), dim3((unsigned)cs->n_huge), dim3(MATVEC_HUGE_THREADS), 0, ctx->ws, csr(cs, 0), csr(cs, 1), csr(cs, 2), zmont, a, b, c,
                      ptr<u64>(cs->long_rows), cs->l + cs->w);
        if (cs->n_long > cs->n_huge)
            ZK_LAUNCH((k_matvec_long<Fr>), dim3(blocks_for(cs->n_long - cs->n_huge, 4)), dim3(256), 0, ctx->ws, csr(cs, 0), csr(cs, 1), csr(cs, 2), zmont, a, b, c,
                      ptr<u64>(cs->long_rows) + cs->n_huge, cs->n_long - cs->n_huge, cs->l + cs->w);
    }
    static unsigned gmax_rows(const int g[3]) { return (unsigned)std::max(g[0], std::max(g[1], g[2])); }

    // K1-K4 on the device: leaves h (canonical integers, sigma order) in ctx->cur->va.  The three vectors a, b, c live
    // back to back in va and go through every pass together (one launch per pass, grid.y = 3).
    // `bound`: the key is bound to this system (PkLoader::bind) — the transforms that lead from the quotient's evaluations to h's
    // coefficients, and everything c needs, were applied to the key's bases once: what is left per proof is a and b to their
    // coefficients and on to the coset (FOUR transforms), and U_j = a_j b_j / Z(g) as canonical integers in NATURAL order in va.
    // `check` (checked mode): a b == c over the R1CS rows is tested where all three vectors exist and BEFORE the first transform,
    // which works in place, is enqueued behind it on the same stream; over a bound key that means C's mat-vec as well.
    static void witness_map(zkhip_ctx* ctx, const zkhip_r1cs* cs, NttPlan<C>* pl, bool bound = false, int half = -1, bool check = false) {
        Stream s = ctx->ws;
        const u64 N = pl->N;
        ctx->cur->va.ensure(3 * N * sizeof(Fr));
        Fr *a = ptr<Fr>(ctx->cur->va), *b = a + N, *c = b + N;
        if (half >= 0) {
            // ONE of the two vectors a bound key's proof needs on the coset (a member of a multi-GPU proof: its partner of the other
            // parity computes the other, Prover::enqueue_tail multiplies them once both are here): two transforms instead of four
            Fr* v = a + (u64)half * N;
            matvec(ctx, cs, ptr<Fr>(ctx->cur->zmont), a, b, c, cs->n, cs->l, N, 1, half);
            event_record(ctx->cur->ntt_b, s);
            Tr::ntt_kind_a(ctx, pl, v, true, ptr<Fr>(pl->s_coset), 1, 0);
            Tr::ntt_kind_b(ctx, pl, v, false, nullptr, 1, 0);
            event_record(ctx->cur->ntt_e, s);
            return;
        }
        matvec(ctx, cs, ptr<Fr>(ctx->cur->zmont), a, b, c, cs->n, cs->l, N, (bound && !check) ? 2 : 3);
        if (check) enqueue_check(*ctx->cur, a, b, c, cs->n, s);
        event_record(ctx->cur->ntt_b, s);
        // SIX transforms (the reference's witness_map runs seven; FOUR over a bound key): ntt_quotient, a and b through every pass together.
        // Same h, bit for bit.
        Tr::ntt_quotient(ctx, pl, a, 2, c, bound, [&](const Fr& zinv) {
            ZK_LAUNCH((k_quotient<typename Fr::Params>), dim3(blocks_for(N, 256)), dim3(256), 0, s, a, b, zinv, a, N);
        });
        event_record(ctx->cur->ntt_e, s);
    }

    // ---- checked mode (zkhip_ctx_set_checked).  The slot's verdict is reset where its zflag word is, tested by k_r1cs_check on the
    // stream that owns the three row-product vectors, travels in the slot's pinned record behind the zflag word (copy_out) and is
    // read where that word is read (unsatisfied): no synchronisation of its own.
    static void verdict_reset(ProofSlot& sl, Stream st) {
        sl.verdict.ensure(16);
        dev_memset(sl.verdict.p, 0xff, 8, st);
        dev_memset((uint8_t*)sl.verdict.p + 8, 0, 8, st);
    }
    static void enqueue_check(ProofSlot& sl, const Fr* a, const Fr* b, const Fr* c, u64 n, Stream s) {
        ZK_LAUNCH((k_r1cs_check<typename Fr::Params>), dim3(blocks_for(n, 256)), dim3(256), 0, s, a, b, c, n, ptr<unsigned long long>(sl.verdict));
    }
    // the slot's finished proof failed its check: noted in the context
    static bool unsatisfied(zkhip_ctx* ctx, const ProofSlot& sl, const Lay& ly) {
        if (sl.check_idx < 0) return false;
        u64 v[2];
        memcpy(v, ly.verdict(sl), 16);
        if (!v[1]) return false;
        ctx->unsat.push_back({(u32)sl.check_idx, v[0], v[1]});
        return true;
    }
    // the end of a checked prove call of `count` proofs over `cs`: ZKHIP_ERR_UNSATISFIED naming the first proof that failed
    static void raise_unsatisfied(const zkhip_ctx* ctx, u32 count, const zkhip_r1cs* cs) {
        if (ctx->unsat.empty()) return;
        const auto& u = ctx->unsat.front();
        char msg[200];
        snprintf(msg, sizeof(msg), "proof %u of %u: constraint %llu of %llu is not satisfied (%llu in all)", u.proof, count, (unsigned long long)u.first_row,
                 (unsigned long long)cs->n, (unsigned long long)u.n_bad);
        throw ApiError{ZKHIP_ERR_UNSATISFIED, msg};
    }
    // zkhip_r1cs_check: the three mat-vecs over rows [0, n) and the test, nothing else; out = {lowest failing row or ~0, failing rows}
    static void r1cs_check(zkhip_ctx* ctx, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, u64 out[2]) {
        ProofSlot& sl = *ctx->cur;
        Stream s = ctx->stream;
        ctx->ws = s;
        const u64 m = cs->l + cs->w, n = cs->n;
        const Fr* z = stage_z(ctx, sl, m, m + 2, z_host, z_dev, true, true);
        sl.zmont.ensure(m * 32);
        // canonical integer -> R'-form (NttPlan::k_to_rp, without a plan: the stand-alone check transforms nothing)
        ZK_LAUNCH((k_mul_const<Fr>), dim3(blocks_for(m, 256)), dim3(256), 0, s, z, ptr<Fr>(sl.zmont), m, fe_to_mont(rp_factor<Fr>()));
        sl.vc.ensure(3 * std::max<u64>(n, 1) * sizeof(Fr));
        Fr *ra = ptr<Fr>(sl.vc), *rb = ra + n, *rc = rb + n;
        if (n) matvec(ctx, cs, ptr<Fr>(sl.zmont), ra, rb, rc, n, 0, n);
        enqueue_check(sl, ra, rb, rc, n, s);
        u32 flag = 0;
        dev_d2h(&flag, sl.zflag.p, 4, s);
        dev_d2h(out, sl.verdict.p, 16, s);
        stream_sync(s);
        require_canonical(flag);
    }

    // z -> HBM (canonical integers) into a buffer of `cap` entries: the prover's hold what it appends to the m of the assignment (the
    // blinding pair; GM17: the extension)
    static void upload_z(zkhip_ctx* ctx, DBuf& dst, u64 m, u64 cap, const uint8_t* z, DBuf& flag) {
        Fr z0 = fe_from_bytes_canon<Fr>(z);
        Fr one = Fr::zero(); one.v[0] = 1;
        require(z0.equals(one), ZKHIP_ERR_BAD_ARG, Z0_NOT_ONE_MSG);
        dst.ensure(cap * 32);
        dev_h2d(dst.p, z, m * 32, ctx->stream);
        // every entry must be a canonical field element (checked on the device; the verdict is read with the results)
        flag.ensure(4);
        dev_memset(flag.p, 0, 4, ctx->stream);
        ZK_LAUNCH((k_check_canonical<Fr>), dim3(blocks_for(m, 256)), dim3(256), 0, ctx->stream, ptr<Fr>(dst), m, ptr<u32>(flag));
    }
    // the same from the packed form (validated on the host: zkhip_api.hip) into a buffer of `cap` entries: one copy of the packed bytes
    // into the context's buffer, one launch that widens them and tests the 32-byte values against r, the same verdict word.
    // ctx->zpack stays ONE buffer however many packed proofs are in flight: the copy in, the widening kernel and the next proof's copy in
    // are all enqueued on ctx->stream, so the kernel has read the bytes of proof t before the copy of proof t + 1 overwrites them, and
    // nothing else ever reads them (every later stage works from the slot's scalars).  Growing it frees the old buffer, which waits
    // for the device: a larger packed buffer than any before costs that once.
    static void unpack_z(zkhip_ctx* ctx, DBuf& dst, u64 m, u64 cap, const PackedZ& zp, DBuf& flag) {
        Stream s = ctx->stream;
        dst.ensure(cap * 32);
        ctx->zpack.ensure(zp.len);
        dev_h2d(ctx->zpack.p, zp.bytes, zp.len, s);
        flag.ensure(4);
        dev_memset(flag.p, 0, 4, s);
        const uint8_t* d = ptr<uint8_t>(ctx->zpack);
        ZK_LAUNCH((k_unpack_assignment<Fr>), dim3(blocks_for(m, ZPACK_BLOCK_ELEMS)), dim3(256), 0, s, d + zp.tags_off, (const u64*)(d + zp.index_off),
                  d + zp.payload_off, ptr<Fr>(dst), m, ptr<u32>(flag));
    }
    // the same from the bytes of a witness file (framing checked on the host: witness_header_validate) into a buffer of `cap` entries:
    // one copy of the file into the context's buffer, k_witness_claim over its entries, k_witness_gather over the columns.  `flag`
    // becomes 16 bytes: the verdict word (bit 0 is never set on this route: every value is tested where it is claimed), a pad, and
    // the lowest missing column as a u64.
    // ctx->wraw and ctx->wowner stay ONE buffer each however many witness proofs are in flight, by the argument of ctx->zpack: the
    // copy in, the clearing of `owner`, the two launches and the next proof's copy in are all enqueued on ctx->stream, so the gather
    // has read the bytes and the owners of proof t before the copy and the memset of proof t + 1 overwrite them, and nothing else
    // ever reads either (every later stage works from the slot's scalars; the slot's verdict words and its pinned head of z are its
    // own).  Growing one frees the old buffer, which waits for the device: a longer file than any before costs that once.
    // `owner` is cleared by a memset per ingest rather than tagged with a generation number: a tag would take bits from the 32 that
    // hold entry + 1 (a file may have 2^32 - 2 entries), and the memset is m x 4 bytes beside a copy of 40 bytes per entry.
    static void ingest_z(zkhip_ctx* ctx, DBuf& dst, u64 m, u64 cap, const WitnessZ& wz, DBuf& flag) {
        Stream s = ctx->stream;
        const zkhip_wplan* plan = wz.plan;
        const u64 slots = (wz.len + 15) / 16;
        dst.ensure(cap * 32);
        ctx->wraw.ensure(slots * 16);
        ctx->wowner.ensure(m * 4);
        dev_h2d(ctx->wraw.p, wz.bytes, wz.len, s);
        dev_memset(ctx->wowner.p, 0, m * 4, s);
        flag.ensure(16);
        dev_memset(flag.p, 0, 8, s);
        dev_memset((uint8_t*)flag.p + 8, 0xff, 8, s);
        ZK_LAUNCH((k_witness_claim<Fr>), dim3(blocks_for(wz.count, WIT_BLOCK)), dim3(WIT_BLOCK), 0, s, ptr<uint4>(ctx->wraw), slots, wz.count, ptr<u32>(plan->pos),
                  (u64)plan->host->pos.size(), ptr<u32>(plan->neg), (u64)plan->host->neg.size(), witness_id_bound(wz.count), ptr<u32>(ctx->wowner), ptr<u32>(flag));
        ZK_LAUNCH((k_witness_gather<Fr>), dim3(blocks_for(m, WIT_BLOCK)), dim3(WIT_BLOCK), 0, s, ptr<uint8_t>(ctx->wraw), ptr<u32>(ctx->wowner), ptr<Fr>(dst), m,
                  ptr<u32>(flag), (unsigned long long*)((uint8_t*)flag.p + 8));
    }
    // what the verdict words of a slot say (flag, lowest missing column): the host reader's errors for a witness file, the message of
    // zkhip_prove_g16 for an entry of a host or packed assignment that is not canonical.  A PARSE condition wins over a missing variable
    static void require_verdict(u32 flag, u32 low, const WPlanTables* wit) {
        require(!(flag & WIT_FLAG_NON_CANONICAL), ZKHIP_ERR_PARSE, "non-canonical field element in the witness");
        require(!(flag & WIT_FLAG_ID_RANGE), ZKHIP_ERR_PARSE, "variable id out of range in the witness");
        if (flag & WIT_FLAG_MISSING) {
            const std::string name = wit && low < wit->order.size() ? witness_var_name(wit->order[low]) : "column " + std::to_string(low);
            throw ApiError{ZKHIP_ERR_UNSATISFIED, "assignment missing for variable " + name};
        }
        require_canonical(flag);
    }
    static void require_verdict(const ProofSlot& sl, const Lay& ly) {
        u32 low = 0;
        memcpy(&low, ly.zflag(sl) + 4, 4);
        require_verdict(ly.zflag_word(sl), low, sl.wit.get());
    }
    // the assignment into the slot, from host memory or from a resident one (checked when it was uploaded: a clean zflag word), and
    // the verdict of a checked proof reset behind it.  Returns where it is: a resident one stays where it was if the caller only
    // reads it (`in_place`; the provers append to theirs)
    // (`zp`: the assignment comes packed — zkhip_queue_submit_packed — and is widened into the slot; its verdict word is the slot's)
    // (`wz`: the assignment comes as a witness file — zkhip_queue_submit_witness — and is ordered into the slot; its verdict words are
    // the slot's, and the head of z, where the public inputs are, is copied to the slot's pinned buffer on the stream that wrote it)
    static const Fr* stage_z(zkhip_ctx* ctx, ProofSlot& sl, u64 m, u64 cap, const uint8_t* z_host, const void* z_dev, bool checked, bool in_place = false,
                             const PackedZ* zp = nullptr, const WitnessZ* wz = nullptr) {
        Stream st = ctx->stream;
        sl.wit.reset();
        if (wz) {
            const u64 l = wz->plan->host->l;
            if (sl.h_inputs_cap < l * 32) {
                host_free_pinned(sl.h_inputs);
                sl.h_inputs = nullptr; sl.h_inputs_cap = 0;
                sl.h_inputs = host_alloc_pinned(l * 32);
                sl.h_inputs_cap = l * 32;
            }
            ingest_z(ctx, sl.scalars, m, cap, *wz, sl.zflag);
            dev_d2h_pinned(sl.h_inputs, sl.scalars.p, l * 32, st);
            sl.wit = wz->plan->host;
            if (checked) verdict_reset(sl, st);
            return ptr<Fr>(sl.scalars);
        }
        if (zp) {
            unpack_z(ctx, sl.scalars, m, cap, *zp, sl.zflag);
            if (checked) verdict_reset(sl, st);
            return ptr<Fr>(sl.scalars);
        }
        if (z_host) {
            upload_z(ctx, sl.scalars, m, cap, z_host, sl.zflag);
        } else {
            if (!in_place) {
                sl.scalars.ensure(cap * 32);
                dev_d2d(sl.scalars.p, z_dev, m * 32, st);
            }
            sl.zflag.ensure(4);
            dev_memset(sl.zflag.p, 0, 4, st);
        }
        if (checked) verdict_reset(sl, st);
        return (z_host || !in_place) ? ptr<Fr>(sl.scalars) : (const Fr*)z_dev;
    }
    static void require_canonical(u32 flag) {
        require(flag == 0, ZKHIP_ERR_BAD_ARG, "an assignment entry is not a canonical field element (>= r)");
    }
    // r, s into the tail slots; Montgomery copy of z for the mat-vec
    static void stage_scalars(zkhip_ctx* ctx, NttPlan<C>* pl, void* d_scalars, u64 m, const uint8_t* r, const uint8_t* s_) {
        Stream s = ctx->stream;
        ctx->cur->zmont.ensure(m * 32);
        dev_h2d((uint8_t*)d_scalars + m * 32, r, 32, s);
        dev_h2d((uint8_t*)d_scalars + (m + 1) * 32, s_, 32, s);
        // z in R'-form for the mat-vec (the matrices' values stay in the saturated Montgomery form: their product is R'-form)
        ZK_LAUNCH((k_mul_const<Fr>), dim3(blocks_for(m, 256)), dim3(256), 0, s, (const Fr*)d_scalars, ptr<Fr>(ctx->cur->zmont), m, pl->k_to_rp);
    }

    // ---- enqueue: every kernel and copy of one proof, no host synchronisation.  Both schemes run the same machine — the assignment
    // and the blinding scalars staged into a slot (open_slot, stage_z), the digits of S = [z.., r, s] sorted once and the G2 lane
    // started (start_z_lanes), a witness map of the scheme's own on a second stream, the G1 lanes over z released when h is ready,
    // the H lane, the copies out (lanes_after_h) — and differ in the middle: Groth16's is witness_map below, GM17's Gm17::enqueue.
    // z_dev != nullptr: the assignment is already in HBM (copied device-to-device into the slot); else z is a host buffer
    // `lone`: nothing else of this context is in flight beside this proof (the single-proof entry points; a batch pipelines)
    static void enqueue(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev,
                        const uint8_t* r, const uint8_t* s_, bool lone = false, int check_idx = -1, const PackedZ* zp = nullptr,
                        const WitnessZ* wz = nullptr) {
        enqueue_head(ctx, sl, pk, cs, z_host, z_dev, r, s_, lone, -1, check_idx, zp, wz);
        enqueue_tail(ctx, sl, pk, cs);
    }
    // whether a proof over (pk, cs) may be split between members: a bound key (its proof needs a and b on the coset and nothing else
    // of the witness map) over a domain where two transforms cost more than the exchange
    static bool can_split(const zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs) {
        return pk->scheme == 0 && is_bound(pk, cs) && pk->logN >= ctx->split_min_log;
    }
    static bool is_bound(const zkhip_pk* pk, const zkhip_r1cs* cs) { return pk->bound_uid != 0 && pk->bound_uid == cs->uid; }   // (zkhip_pk_bind_r1cs; a shard: its ranges of H' / L')
    // a free slot made the current one, with its streams and events, and the plan of the key's domain
    static NttPlan<C>* open_slot(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk) {
        require(!sl.busy, ZKHIP_ERR_DEVICE, "internal: proof slot still in flight");
        make_pipe_streams(ctx);     // (a resident prover's first proof: every stream of the plan, in pipe order)
        slot_init(ctx, sl);
        NttPlan<C>* pl = get_plan<C>(ctx, pk->logN);
        require(pl->split() == pk->ntt_log1, ZKHIP_ERR_BAD_ARG, "the key's h bases were ordered for another NTT split (NTT_SINGLE_MAX_LOG changed): reload the key");
        sl.t_start = std::chrono::steady_clock::now();
        ctx->cur = &sl;
        ctx->ws = ctx->stream;
        return pl;
    }
    // the staged scalars, the sort of the assignment, the G2 lane and the witness map — all of it (`half` = -1) or the vector `half`
    // (0: a, 1: b) of a bound key's, after which sl.half_ready is recorded and the caller brings the other vector into
    // sl.va + (1 - half) * N before enqueue_tail
    static void enqueue_head(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev,
                             const uint8_t* r, const uint8_t* s_, bool lone, int half, int check_idx = -1, const PackedZ* zp = nullptr,
                             const WitnessZ* wz = nullptr) {
        PkLoader<C>::check_match(pk, cs, 0);
        const bool bound = is_bound(pk, cs);
        require(half < 0 || (bound && half <= 1), ZKHIP_ERR_BAD_ARG, "internal: only a proof over a bound key splits its witness map");
        Fr rr = fe_from_bytes_canon<Fr>(r), ss = fe_from_bytes_canon<Fr>(s_);
        require(canon_lt_mod(rr) && canon_lt_mod(ss), ZKHIP_ERR_BAD_ARG, "r or s not a canonical field element");
        NttPlan<C>* pl = open_slot(ctx, sl, pk);
        sl.half = half;
        sl.lone = lone;
        sl.check_idx = half < 0 ? check_idx : -1;
        memcpy(sl.r, r, 32);
        memcpy(sl.s, s_, 32);
        Stream st = ctx->stream;
        stage_z(ctx, sl, pk->m, pk->m + 2, z_host, z_dev, sl.check_idx >= 0, false, zp, wz);
        stage_scalars(ctx, pl, sl.scalars.p, pk->m, r, s_);
        event_record(sl.ev[0], st);

        // ---- MSMs over S = [z_0..z_{m-1}, r, s]: A, B1, L in G1 and B2 in G2 share one digit/sort pass
        const Lay ly(ctx, pk);
        ly.reserve(sl);
        start_z_lanes(ctx, sl, pk, ly);

        // ---- K1-K4 and the h-sort, on the NTT stream: the main stream is free for the next proof's staging and z-sort
        Stream wn = ctx->serial ? st : slot_ntt_stream(ctx, sl);
        stream_wait_event(wn, sl.ev[0]);
        event_record(sl.ev[1], wn);
        ctx->ws = wn;
        witness_map(ctx, cs, pl, bound, half, sl.check_idx >= 0);
        ctx->ws = ctx->stream;
        if (half >= 0) {
            event_record(sl.half_ready, wn);
            sl.split_pk = pk;
            sl.split_cs = cs;
            sl.split_bound = bound;
            sl.split_pending = true;
        }
    }
    // ... and the rest: (the product of the two halves,) the G1 lanes over z, the h sort and the H MSM, the copies out
    static void enqueue_tail(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const zkhip_r1cs* cs) {
        const u64 N = pk->N;
        ctx->cur = &sl;
        Stream wn = ctx->serial ? ctx->stream : slot_ntt_stream(ctx, sl);
        // where the H MSM's scalars are: the first vector — except for a split proof, whose product goes to the THIRD (c's, idle over a
        // bound key): its own half stays as it is for the partner that may still be copying it
        const u32* h_scalars = ptr<u32>(sl.va) + (sl.half >= 0 ? 2 * N * 8 : 0);
        if (sl.half >= 0) {
            // both vectors are on the coset now (the other one arrived on this stream): U_j = a_j b_j / Z(g), canonical integers
            Fr* a = ptr<Fr>(sl.va);
            ZK_LAUNCH((k_quotient<typename Fr::Params>), dim3(blocks_for(N, 256)), dim3(256), 0, wn, a, a + N, fe_from_mont(get_plan<C>(ctx, pk->logN)->zinv), a + 2 * N, N);
        }
        // (a split proof: what the head saw — the product above pairs with the bound tables whatever has happened to the key since)
        lanes_after_h(ctx, sl, pk, Lay(ctx, pk), sl.half >= 0 ? sl.split_bound : is_bound(pk, cs), sl.lone, h_scalars, wn);
    }

    // ---- the z lanes' start: the digits of S sorted once on the main stream — and once more without the variables a family of
    // tables holds at infinity (zkhip_pk::thin_mask) — and the G2 lane, the longest chain of a proof.
    // An accumulation kernel is sized to fill the machine, saturates the integer multiplier and nothing preempts it:
    // whatever arrives beside it waits for a place or crawls (kernel traces, profiles/r2_single_proof_traces.md: a
    // 0.14 ms mat-vec took 4 ms, a 0.2 ms transform pass 3 ms), h arrives late and the H MSM trails alone behind
    // everything.  So the G2 lane starts at once, the witness map runs beside it, and the G1 lanes over z wait for h
    // (`z_gate`; 2 = the G2 lane waits as well).
    static void start_z_lanes(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const Lay& ly) {
        if (!pk->z_n) return;
        // (a sharded key pairs its index range of the bases with the same range of the scalars)
        const u32* digits = ptr<u32>(sl.scalars) + pk->z_lo * 8;
        msm_prepare(ctx, ctx->stream, sl.sorts[0], digits, ly.shz, pk->z_n);
        if (pk->thin_mask) msm_prepare(ctx, ctx->stream, sl.sorts[2], digits, ly.shz, pk->z_n, ptr<u32>(pk->thin_keep), &sl.sorts[0]);
        if (z_gate(ctx) < 2) run_g2(ctx, sl, pk, ly, nullptr);
    }
    static void run_g2(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const Lay& ly, Event after) {
        const bool thin = pk->thin_mask & 8;   // the list b2_ext pairs with
        msm_run<Fq2>(ctx, sl.lanes[3], sl.sorts[thin ? 2 : 0], pk->b2_ext.p, with_inf(ly.shz, thin ? pk->inf_many_thin[3] : pk->inf_many[3]), ly.ws2(sl),
                     sl.acc_b[4], sl.acc_e[4], after, ly.hs2(sl));
    }
    // ---- the lanes after h: its scalars (canonical integers, the order of the key's h bases) are at `h_scalars`, written on `wn`.
    // "h ready" is recorded there; the G2 lane if z_gate held it, the G1 lanes over z, the h sort on `wn` and the H lane, the copies out.
    static void lanes_after_h(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const Lay& ly, bool bound, bool lone, const u32* h_scalars, Stream wn) {
        Stream st = ctx->stream;
        event_record(sl.ev[2], wn);
        if (pk->z_n) {
            const int gate = z_gate(ctx);
            const Event h_ready = gate ? sl.ev[2] : nullptr;
            if (gate >= 2) run_g2(ctx, sl, pk, ly, h_ready);
            // A G2 accumulation at one wave per SIMD (BLS12-381: the wave takes the SIMD's whole register file) shares no SIMD with a
            // G1 wave: G1 workgroups that arrive while some of its workgroups are still waiting for a place take the places, and the
            // G2 lane — the longest chain of such a proof — finishes that much later.  The witness map used to be the head start; a
            // bound key's is a third shorter, and the lone Poseidon proof went from 6.9 to 8.1 ms
            // (profiles/r5k_bound_key_single_proof_latency_ab.txt).  So a LONE proof holds its G1 lanes until the G2 accumulation is
            // through; a batch has other proofs' kernels to fill the machine and is left alone.
            Event g1_after = h_ready;
            constexpr bool g2_owns_simds = MsmTuning<typename Unsat<Fq2>::type>::ACCUM_WPE == 1;
            if (g2_owns_simds && lone && !ctx->serial && (ctx->g2_head_start == 2 || (ctx->g2_head_start == 1 && bound))) {
                if (h_ready) stream_wait_event(st, h_ready);
                stream_wait_event(st, sl.acc_e[4]);
                event_record(sl.g1_go, st);
                g1_after = sl.g1_go;
            }
            run_z_g1(ctx, sl, pk, ly, g1_after, bound);
        } else {
            empty_msm(ctx, sl, ly, true);
        }
        // ---- H = MSM(h bases, h) in their order (sigma; the zero-padded tail pairs with infinity bases.  A bound key: the quotient's
        // evaluations in natural order against H' — the same MSM machinery, other bases)
        if (pk->h_n) {
            msm_prepare(ctx, wn, sl.sorts[1], h_scalars + pk->h_lo * 8, ly.shh, pk->h_n);
            msm_run<Fq>(ctx, sl.lanes[4], sl.sorts[1], bound ? pk->h_bound.p : pk->h_sigma.p, with_inf(ly.shh, bound ? pk->inf_many_bound[1] : pk->inf_many[4]),
                        ly.ws1(sl, 3), sl.acc_b[3], sl.acc_e[3], nullptr, ly.hs1(sl, 3));
        } else {
            empty_msm(ctx, sl, ly, false);
        }
        copy_out(ctx, sl, ly);
    }

    // ---- A, B1, L: the three G1 MSMs over the sorted assignment (window sums to MSMs 0, 1, 2 of ws1)
    // (`bound`: L' in l's place, on the common list whatever l's family is — its public entries are finite)
    static void run_z_g1(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const Lay& ly, Event h_ready, bool bound) {
        const void* tab[3] = {pk->a_ext.p, pk->b1_ext.p, bound ? pk->l_bound.p : pk->l_ext.p};
        auto thin = [&](int k) { return (bound && k == 2) ? 0u : (pk->thin_mask >> k) & 1u; };
        auto inf_many = [&](int k) { return (bound && k == 2) ? pk->inf_many_bound[0] : thin(k) ? pk->inf_many_thin[k] : pk->inf_many[k]; };
        if (!ctx->fuse_z) {
            for (int k = 0; k < 3; ++k)
                msm_run<Fq>(ctx, sl.lanes[k], thin(k) ? sl.sorts[2] : sl.sorts[0], tab[k], with_inf(ly.shz, inf_many(k)), ly.ws1(sl, k), sl.acc_b[k], sl.acc_e[k], h_ready,
                            ly.hs1(sl, k));
            return;
        }
        // One launch per sorted list: the tables on the common list together, the tables on the thinned list together (up to three
        // tables on one, none on the other).  The first table of a group lends its lane; the others ride on its launches.
        for (u32 which = 0; which < 2; ++which) {
            int member[3], nm = 0;
            for (int k = 0; k < 3; ++k)
                if (thin(k) == which) member[nm++] = k;
            if (!nm) continue;
            const int lead = member[0];
            const void* tabs[3];
            bool many = false;
            for (int q = 0; q < nm; ++q) { tabs[q] = tab[member[q]]; many = many || inf_many(member[q]); }
            // destination slots: lead, then every `step` slots (any subset of {0, 1, 2} is an arithmetic progression)
            const int step = nm > 1 ? member[1] - member[0] : 1;
            msm_run_tables<Fq>(ctx, sl.lanes[lead], which ? sl.sorts[2] : sl.sorts[0], tabs, nm, with_inf(ly.shz, many), ly.ws1(sl, lead), (u32)(step * ly.Wmax),
                               sl.acc_b[lead], sl.acc_e[lead], h_ready, ly.hs1(sl, lead));
            Stream s0 = ctx->serial ? ctx->stream : lane_stream(sl.lanes[lead]);
            for (int q = 1; q < nm; ++q) {
                event_record(sl.acc_b[member[q]], s0);
                event_record(sl.acc_e[member[q]], s0);
                event_record(sl.lanes[member[q]].done, s0);
            }
        }
    }

    // ---- the end of a proof's device work: every lane has copied its window sums out behind its fold (msm_run_tables) and recorded
    // `done`; a stream of its own — the main stream is free for the next proof — waits for all of them, fetches the verdict of the
    // canonical check and records "all done"
    static void copy_out(zkhip_ctx* ctx, ProofSlot& sl, const Lay& ly) {
        Stream st = ctx->stream;
        Stream so = ctx->serial ? st : ctx_out_stream(ctx);
        for (int k = 0; k < ZK_NLANES; ++k) stream_wait_event(so, sl.lanes[k].done);
        sl.zflag.ensure(4);
        dev_d2h_pinned(ly.zflag(sl), sl.zflag.p, 4, so);   // written on the main stream before ev[0], which every lane waits for
        if (sl.wit) dev_d2h_pinned(ly.zflag(sl) + 4, (const uint8_t*)sl.zflag.p + 8, 4, so);   // (a witness file: the lowest missing column — below 2^32 — beside it)
        if (sl.check_idx >= 0) {
            stream_wait_event(so, sl.ev[2]);      // "h ready": recorded behind the check on the stream of the witness map
            dev_d2h_pinned(ly.verdict(sl), sl.verdict.p, 16, so);
        }
        event_record(sl.ev[3], so);
        sl.busy = true;
    }

    // a rank whose range is empty (more ranks than points): all-infinity window sums on the device and in the host mirror (nothing is
    // in flight for them), events recorded so that the bookkeeping of the slot stays uniform.  `over_z`: the four lanes over z, else H's
    static void empty_msm(zkhip_ctx* ctx, ProofSlot& sl, const Lay& ly, bool over_z) {
        Stream st = ctx->stream;
        const int k0 = over_z ? 0 : 3, nk = over_z ? 3 : 1;
        dev_memset(ly.ws1(sl, k0), 0, nk * ly.lane_bytes(), st);
        memset(ly.hs1(sl, k0), 0, nk * ly.lane_bytes());
        if (over_z) {
            dev_memset(ly.ws2(sl), 0, ly.b2(), st);
            memset(ly.hs2(sl), 0, ly.b2());
        }
        for (int k = over_z ? 0 : 4; k < (over_z ? 4 : 5); ++k) {
            const int e = k == 3 ? 4 : k == 4 ? 3 : k;   // lane 3 (B2) times with event pair 4, lane 4 (H) with pair 3
            event_record(sl.acc_b[e], st);
            event_record(sl.acc_e[e], st);
            event_record(sl.lanes[k].done, st);
        }
    }

    // the five MSM results of a proof (or of one rank's share of it)
    struct Sums {
        Xyzz<Fq> a, b1, l, h;
        Xyzz<Fq2> b2;
    };
    // ---- wait for the slot's proof; Horner over its window sums
    static Sums collect(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk) {
        require(sl.busy, ZKHIP_ERR_DEVICE, "internal: no proof in flight in this slot");
        event_sync(sl.ev[3]);
        sl.busy = false;
        split_clear(sl);
        const Lay ly(ctx, pk);
        require_verdict(sl, ly);
        // five independent Horner chains (W x c doublings each): one host thread per MSM, the G2 chain on this one
        Sums g;
        HostThreads th;
        th.run([&] { g.a = msm_combine(ly.hs1(sl, 0), ly.shz); });
        th.run([&] { g.b1 = msm_combine(ly.hs1(sl, 1), ly.shz); });
        th.run([&] { g.l = msm_combine(ly.hs1(sl, 2), ly.shz); });
        th.run([&] { g.h = msm_combine(ly.hs1(sl, 3), ly.shh); });
        g.b2 = msm_combine(ly.hs2(sl), ly.shz);
        th.join();
        return g;
    }
    // ---- K9: C = s*A + r*B1 - rs*delta_1 + L + H   (App. A.3; alpha/beta/delta terms already inside A, B1, B2)
    static void assemble(const zkhip_pk* pk, const Sums& g, const uint8_t* r, const uint8_t* s_, uint8_t* out) {
        const Fr rr = fe_from_bytes_canon<Fr>(r), ss = fe_from_bytes_canon<Fr>(s_);
        // three independent 254-bit scalar multiplications
        Xyzz<Fq> sA, rB1, rsD;
        {
            HostThreads th;
            th.run([&] { sA = xyzz_mul_limbs(g.a, ss.v, Fr::N); });
            th.run([&] { rB1 = xyzz_mul_limbs(g.b1, rr.v, Fr::N); });
            rsD = rs_delta(pk, rr, ss);
        }
        assemble_tail(g, sA, rB1, rsD, out);
    }
    static void assemble_tail(const Sums& g, const Xyzz<Fq>& sA, const Xyzz<Fq>& rB1, const Xyzz<Fq>& rsD, uint8_t* out) {
        Xyzz<Fq> gC = xyzz_add(sA, rB1);
        gC = xyzz_add(gC, xyzz_neg(rsD));
        gC = xyzz_add(gC, g.l);
        gC = xyzz_add(gC, g.h);
        Aff<Fq> pa, pc;
        Aff<Fq2> pb;
        {
            HostThreads th;               // three inversions: one thread each
            th.run([&] { pa = xyzz_to_affine(g.a); });
            th.run([&] { pc = xyzz_to_affine(gC); });
            pb = xyzz_to_affine(g.b2);
        }
        write_proof(g.a.is_inf(), pa, g.b2.is_inf(), pb, gC.is_inf(), pc, out);
    }
    // the proof as both schemes write it: A (G1), B (G2), C (G1) as canonical affine coordinates, and a flag per point at infinity
    static void write_proof(bool inf_a, const Aff<Fq>& pa, bool inf_b, const Aff<Fq2>& pb, bool inf_c, const Aff<Fq>& pc, uint8_t* out) {
        memset(out, 0, PROOF_BYTES);
        if (!inf_a) { write_fe(pa.x, out); write_fe(pa.y, out + FQB); }
        if (!inf_b) {
            write_fe(pb.x.c0, out + 2 * FQB); write_fe(pb.x.c1, out + 3 * FQB);
            write_fe(pb.y.c0, out + 4 * FQB); write_fe(pb.y.c1, out + 5 * FQB);
        }
        if (!inf_c) { write_fe(pc.x, out + 6 * FQB); write_fe(pc.y, out + 7 * FQB); }
        out[8 * FQB] = inf_a; out[8 * FQB + 1] = inf_b; out[8 * FQB + 2] = inf_c;
    }
    static constexpr size_t PROOF_BYTES = 8 * FQB + 3;
    static void fill_timings(ProofSlot& sl, zkhip_timings* tm, std::chrono::steady_clock::time_point t_fin) {
        const auto t_end = std::chrono::steady_clock::now();
        if (tm) {
            memset(tm, 0, sizeof(*tm));
            // the five MSMs run on their own streams, concurrently with each other and with the NTT pipeline:
            // msm_z = staging done -> last of A/B1/L/B2 finished; msm_h = h ready -> H finished (overlapping intervals)
            for (int k = 0; k < 4; ++k) tm->msm_z_ms = std::max(tm->msm_z_ms, event_elapsed_ms(sl.ev[0], sl.lanes[k].done));
            tm->ntt_ms = event_elapsed_ms(sl.ev[1], sl.ev[2]);   // matvec + 7 transforms + quotient
            tm->kernel_ntt_ms = event_elapsed_ms(sl.ntt_b, sl.ntt_e);   // the transform passes and the quotient kernel only
            tm->msm_h_ms = event_elapsed_ms(sl.ev[2], sl.lanes[4].done);
            tm->finish_ms = std::chrono::duration<float, std::milli>(t_end - t_fin).count();
            tm->total_ms = std::chrono::duration<float, std::milli>(t_end - sl.t_start).count();
            for (int k = 0; k < 4; ++k) tm->kernel_msm_accum_g1_ms += event_elapsed_ms(sl.acc_b[k], sl.acc_e[k]);
            tm->kernel_msm_accum_g2_ms = event_elapsed_ms(sl.acc_b[4], sl.acc_e[4]);
        }
    }
    // ---- the host's share of a proof, taken in the order the lanes deliver: r s delta_1 needs nothing of the device, s A and r B1 wait
    // for the lanes over z only — three 254-bit scalar multiplications (0.2 ms) that used to start after the LAST lane and now run
    // beside the H MSM's tail; what is left behind the last event is two group additions and three conversions to affine form
    static void finish(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, uint8_t* out, zkhip_timings* tm) {
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_g16_partial + zkhip_combine_g16");
        require(sl.busy, ZKHIP_ERR_DEVICE, "internal: no proof in flight in this slot");
        const Lay ly(ctx, pk);
        const Fr rr = fe_from_bytes_canon<Fr>(sl.r), ss = fe_from_bytes_canon<Fr>(sl.s);
        Sums g;
        Xyzz<Fq> sA, rB1, rsD;
        std::chrono::steady_clock::time_point t_fin;
        try {
            HostThreads th;
            th.run([&] { rsD = rs_delta(pk, rr, ss); });
            event_sync(sl.lanes[3].done);
            g.b2 = msm_combine(ly.hs2(sl), ly.shz);
            for (int k = 0; k < 3; ++k) event_sync(sl.lanes[k].done);
            g.a = msm_combine(ly.hs1(sl, 0), ly.shz);
            g.b1 = msm_combine(ly.hs1(sl, 1), ly.shz);
            th.run([&] { sA = xyzz_mul_limbs(g.a, ss.v, Fr::N); });
            th.run([&] { rB1 = xyzz_mul_limbs(g.b1, rr.v, Fr::N); });
            g.l = msm_combine(ly.hs1(sl, 2), ly.shz);
            event_sync(sl.lanes[4].done);
            t_fin = std::chrono::steady_clock::now();
            g.h = msm_combine(ly.hs1(sl, 3), ly.shh);
            event_sync(sl.ev[3]);
            th.join();
        } catch (...) {
            sl.busy = false;
            throw;
        }
        sl.busy = false;
        require_verdict(sl, ly);
        if (unsatisfied(ctx, sl, ly)) memset(out, 0, PROOF_BYTES);      // a refused proof: all zero
        else assemble_tail(g, sA, rB1, rsD, out);
        fill_timings(sl, tm, t_fin);
    }
    static Xyzz<Fq> rs_delta(const zkhip_pk* pk, const Fr& rr, const Fr& ss) {
        const Fr rs = fe_from_mont(fe_mul(fe_to_mont(rr), fe_to_mont(ss)));
        uint8_t dec[2 * FQB];
        decode_point<FQB, 2>(pk->delta_g1_canon.data(), dec);
        Aff<Fq> d1;
        memcpy(&d1, dec, sizeof(d1));
        d1 = PkLoader<C>::to_mont_point(d1);
        return xyzz_mul_limbs(Xyzz<Fq>::from_affine(d1), rs.v, Fr::N);
    }
    // The canonical representative of a group element as an XYZZ record: affine coordinates with ZZ = ZZZ = 1 (Montgomery
    // one), infinity all-zero.  The projective coordinates an MSM leaves depend on the order in which the bucket sort's
    // atomics placed the points, i.e. they vary from run to run and from machine to machine while the group element does
    // not; records that cross a process or machine boundary (zkhip_prove_*_partial) are therefore normalised first, so that
    // equal partial sums are equal bytes.  Five host inversions per proof share.
    template <class F>
    static Xyzz<F> canonical(const Xyzz<F>& p) {
        if (p.is_inf()) return Xyzz<F>::inf();
        const Aff<F> a = xyzz_to_affine(p);
        return {a.x, a.y, F::one(), F::one()};
    }
    // one rank's share of the proof in flight in `sl`: the five partial sums as canonical XYZZ records (saturated Montgomery limbs)
    static void emit_partial(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, uint8_t* partial_out, zkhip_timings* tm) {
        Sums g = collect(ctx, sl, pk);
        const auto t_fin = std::chrono::steady_clock::now();
        HostThreads th;
        th.run([&] { g.a = canonical(g.a); });
        th.run([&] { g.b1 = canonical(g.b1); });
        th.run([&] { g.l = canonical(g.l); });
        th.run([&] { g.h = canonical(g.h); });
        g.b2 = canonical(g.b2);
        th.join();
        memcpy(partial_out, &g, sizeof(g));
        fill_timings(sl, tm, t_fin);
    }
    static void prove_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const uint8_t* r,
                              const uint8_t* s_, uint8_t* partial_out, zkhip_timings* tm) {
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, z_dev, r, s_);
        emit_partial(ctx, ctx->slots[0], pk, partial_out, tm);
    }
    // ---- a member's share of a proof whose witness map is SPLIT between the members (a bound key: the proof needs a and b on the
    // coset; the members of even rank transform a, those of odd rank b, and partners exchange — north_star's "NTT domain shard"):
    //   split_begin     the head with this member's half;
    //   split_fetch*    the partner's half into this member's vectors (device to device across xGMI / from host memory);
    //   split_half_out  this member's half to host memory (the multi-process exchange);
    //   split_end_*     the tail, and the member's result as prove_partial / prove_device_sums leave it.
    static void split_begin(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const uint8_t* r,
                            const uint8_t* s_, int half) {
        require(is_bound(pk, cs) && pk->scheme == 0 && (half == 0 || half == 1), ZKHIP_ERR_BAD_ARG,
                "only a Groth16 proof over a key bound to its constraint system splits its witness map (half = 0: a, 1: b)");
        enqueue_head(ctx, ctx->slots[0], pk, cs, z_host, z_dev, r, s_, false, half);
    }
    static const void* split_half_ptr(zkhip_ctx* ctx, const zkhip_pk* pk, int half) { return ptr<Fr>(ctx->slots[0].va) + (u64)half * pk->N; }
    // a collected (or abandoned) split proof: the slot is an ordinary free slot again
    static void split_clear(ProofSlot& sl) {
        sl.split_pending = false;
        sl.split_pk = nullptr;
        sl.split_cs = nullptr;
        sl.half = -1;
    }
    // the slot of the pending split proof — which must be the proof of these handles —, and the stream its halves travel on
    static ProofSlot& split_slot(zkhip_ctx* ctx, const zkhip_pk* pk, Stream* wn = nullptr) {
        ProofSlot& s0 = ctx->slots[0];
        require(s0.split_pending && s0.half >= 0, ZKHIP_ERR_BAD_ARG, "no split proof pending in this context");
        require(s0.split_pk == pk, ZKHIP_ERR_BAD_ARG, "the split proof pending in this context was begun with another proving key");
        if (wn) *wn = ctx->serial ? ctx->stream : ctx_ntt_stream(ctx);
        return ctx->slots[0];
    }
    static void split_fetch(zkhip_ctx* ctx, const zkhip_pk* pk, const void* src, int src_device, Event src_ready) {
        Stream wn;
        ProofSlot& sl = split_slot(ctx, pk, &wn);
        if (src_ready) event_sync(src_ready);           // (the partner's stream, possibly on another device: waited for on the host)
        dev_copy_between(ptr<Fr>(sl.va) + (u64)(1 - sl.half) * pk->N, ctx->device, src, src_device, pk->N * sizeof(Fr), wn);
    }
    static void split_fetch_host(zkhip_ctx* ctx, const zkhip_pk* pk, const uint8_t* other_half) {
        Stream wn;
        ProofSlot& sl = split_slot(ctx, pk, &wn);
        dev_h2d(ptr<Fr>(sl.va) + (u64)(1 - sl.half) * pk->N, other_half, pk->N * sizeof(Fr), wn);
    }
    static void split_half_out(zkhip_ctx* ctx, const zkhip_pk* pk, uint8_t* out) {
        Stream wn;
        ProofSlot& sl = split_slot(ctx, pk, &wn);
        dev_d2h(out, ptr<Fr>(sl.va) + (u64)sl.half * pk->N, pk->N * sizeof(Fr), wn);
        stream_sync(wn);
    }
    static void split_end_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, uint8_t* partial_out, zkhip_timings* tm) {
        ProofSlot& sl = split_slot(ctx, pk);
        require(sl.split_cs == cs, ZKHIP_ERR_BAD_ARG, "the split proof pending in this context was begun with another constraint system");
        enqueue_tail(ctx, sl, pk, cs);
        emit_partial(ctx, ctx->slots[0], pk, partial_out, tm);
    }
    static void split_end_device_sums(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const void** d_ws1, size_t* b1, const void** d_ws2, size_t* b2,
                                      zkhip_timings* tm) {
        ProofSlot& sl = split_slot(ctx, pk);
        require(sl.split_cs == cs, ZKHIP_ERR_BAD_ARG, "the split proof pending in this context was begun with another constraint system");
        enqueue_tail(ctx, sl, pk, cs);
        hand_out_sums(ctx, ctx->slots[0], pk, d_ws1, b1, d_ws2, b2, tm);
    }
    // ---- a member's share of a proof whose witness map is SHARDED across the members (an UNBOUND Groth16 key; shard_witness_map's
    // four steps, each run on every member before the next on any): between shard_begin and shard_end_* the proof is pending in
    // slot 0 as a split proof is.  The member's h coefficients end where its H MSM reads them — positions [h_lo, h_lo + h_n) of va —
    // so the tail is an ordinary proof's.
    static int can_shard(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, u32 G, u32 k) {
        if (pk->scheme != 0 || is_bound(pk, cs)) return -1;
        const NttPlan<C>* pl = get_plan<C>(ctx, pk->logN);
        return (Tr::shard_ok(pl, G) && pk->h_lo == (u64)k * (pl->N / G) && pk->h_n == pl->N / G) ? pl->split() : -1;
    }
    static void shard_begin(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const uint8_t* r, const uint8_t* s_, u32 G, u32 k) {
        ProofSlot& sl = ctx->slots[0];
        PkLoader<C>::check_match(pk, cs, 0);
        require(z_host && pk->scheme == 0 && !is_bound(pk, cs), ZKHIP_ERR_BAD_ARG, "internal: only a Groth16 proof over an unbound key shards its witness map");
        Fr rr = fe_from_bytes_canon<Fr>(r), ss = fe_from_bytes_canon<Fr>(s_);
        require(canon_lt_mod(rr) && canon_lt_mod(ss), ZKHIP_ERR_BAD_ARG, "r or s not a canonical field element");
        NttPlan<C>* pl = open_slot(ctx, sl, pk);
        sl.half = -1;
        sl.lone = false;
        sl.check_idx = -1;
        memcpy(sl.r, r, 32);
        memcpy(sl.s, s_, 32);
        Stream st = ctx->stream;
        stage_z(ctx, sl, pk->m, pk->m + 2, z_host, nullptr, false);
        stage_scalars(ctx, pl, sl.scalars.p, pk->m, r, s_);
        event_record(sl.ev[0], st);
        const Lay ly(ctx, pk);
        ly.reserve(sl);
        start_z_lanes(ctx, sl, pk, ly);
        Stream wn = ctx->serial ? st : slot_ntt_stream(ctx, sl);
        stream_wait_event(wn, sl.ev[0]);
        event_record(sl.ev[1], wn);
        ctx->ws = wn;
        shard_witness_map(ctx, cs, pl, G, k, 0, nullptr);
        ctx->ws = ctx->stream;
        sl.split_pk = pk;
        sl.split_cs = cs;
        sl.split_bound = false;
        sl.split_pending = true;
    }
    static ProofSlot& shard_slot(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs) {
        ProofSlot& s0 = ctx->slots[0];
        require(s0.split_pending && s0.half < 0 && s0.split_pk == pk && s0.split_cs == cs, ZKHIP_ERR_BAD_ARG, "no sharded proof of these handles pending in this context");
        return s0;
    }
    static void shard_step(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, u32 G, u32 k, int step, zkhip_ctx* const* members) {
        ProofSlot& sl = shard_slot(ctx, pk, cs);
        ctx->cur = &sl;
        ctx->ws = ctx->serial ? ctx->stream : slot_ntt_stream(ctx, sl);
        shard_witness_map(ctx, cs, get_plan<C>(ctx, pk->logN), G, k, step, members);
        ctx->ws = ctx->stream;
    }
    static void shard_end_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, uint8_t* partial_out, zkhip_timings* tm) {
        ProofSlot& sl = shard_slot(ctx, pk, cs);
        enqueue_tail(ctx, sl, pk, cs);
        emit_partial(ctx, ctx->slots[0], pk, partial_out, tm);
    }
    static void shard_end_device_sums(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const void** d_ws1, size_t* b1, const void** d_ws2, size_t* b2,
                                      zkhip_timings* tm) {
        ProofSlot& sl = shard_slot(ctx, pk, cs);
        enqueue_tail(ctx, sl, pk, cs);
        hand_out_sums(ctx, ctx->slots[0], pk, d_ws1, b1, d_ws2, b2, tm);
    }
    // one rank's share of a proof, left ON THE DEVICE: the raw bucket-set sums of its five MSMs (ws1: 4 G1 MSMs x Wmax XYZZ
    // sums, ws2: the G2 MSM), for an exchange that never touches host memory (zkhip_multi_use_rccl: RCCL all-gather over
    // xGMI).  Valid until the slot's next proof.
    static void prove_device_sums(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const uint8_t* r,
                                  const uint8_t* s_, const void** d_ws1, size_t* b1, const void** d_ws2, size_t* b2, zkhip_timings* tm) {
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, nullptr, r, s_);
        hand_out_sums(ctx, ctx->slots[0], pk, d_ws1, b1, d_ws2, b2, tm);
    }
    // wait for the proof in flight in `sl` and hand those sums out
    static void hand_out_sums(zkhip_ctx* ctx, ProofSlot& sl, const zkhip_pk* pk, const void** d_ws1, size_t* b1, const void** d_ws2, size_t* b2,
                              zkhip_timings* tm) {
        require(sl.busy, ZKHIP_ERR_DEVICE, "internal: no proof in flight in this slot");
        event_sync(sl.ev[3]);
        sl.busy = false;
        split_clear(sl);
        const Lay ly(ctx, pk);
        *b1 = ly.b1();
        *b2 = ly.b2();
        require_canonical(ly.zflag_word(sl));
        *d_ws1 = sl.ws1.p;
        *d_ws2 = sl.ws2.p;
        fill_timings(sl, tm, std::chrono::steady_clock::now());
    }
    // the same sums, gathered into host memory (one rank's ws1 | ws2), as a partial record for `combine` (not canonical:
    // these never leave the process)
    static void record_from_sums(zkhip_ctx* ctx, const zkhip_pk* pk, const uint8_t* ws1, const uint8_t* ws2, uint8_t* record_out) {
        const Lay ly(ctx, pk);
        std::vector<Xyzz<Fq>> a1(ly.b1() / sizeof(Xyzz<Fq>));
        std::vector<Xyzz<Fq2>> a2(ly.b2() / sizeof(Xyzz<Fq2>));
        memcpy(a1.data(), ws1, ly.b1());
        memcpy(a2.data(), ws2, ly.b2());
        Sums g;
        g.a = msm_combine(ly.lane(a1.data(), 0), ly.shz);
        g.b1 = msm_combine(ly.lane(a1.data(), 1), ly.shz);
        g.l = msm_combine(ly.lane(a1.data(), 2), ly.shz);
        g.h = msm_combine(ly.lane(a1.data(), 3), ly.shh);
        g.b2 = msm_combine(a2.data(), ly.shz);
        memcpy(record_out, &g, sizeof(g));
    }
    // sum of the ranks' partial results ...
    static Sums sum_partials(u32 count, const uint8_t* partials) {
        Sums t;
        t.a = t.b1 = t.l = t.h = Xyzz<Fq>::inf();
        t.b2 = Xyzz<Fq2>::inf();
        for (u32 i = 0; i < count; ++i) {
            Sums g;
            memcpy(&g, partials + (size_t)i * sizeof(Sums), sizeof(g));
            t.a = xyzz_add(t.a, g.a); t.b1 = xyzz_add(t.b1, g.b1); t.l = xyzz_add(t.l, g.l); t.h = xyzz_add(t.h, g.h);
            t.b2 = xyzz_add(t.b2, g.b2);
        }
        return t;
    }
    // ... then the assembly
    static void combine(const zkhip_pk* pk, u32 count, const uint8_t* partials, const uint8_t* r, const uint8_t* s_, uint8_t* out) {
        const Sums t = sum_partials(count, partials);
        Fr rr = fe_from_bytes_canon<Fr>(r), ss = fe_from_bytes_canon<Fr>(s_);
        require(canon_lt_mod(rr) && canon_lt_mod(ss), ZKHIP_ERR_BAD_ARG, "r or s not a canonical field element");
        assemble(pk, t, r, s_, out);
    }
    static constexpr size_t PARTIAL_BYTES = sizeof(Sums);

    // one proof, from a host assignment (`z_host`) or from one resident in HBM (`z_dev`)
    static void prove(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, const uint8_t* z_host, const void* z_dev, const uint8_t* r, const uint8_t* s_,
                      uint8_t* out, zkhip_timings* tm) {
        ctx->unsat.clear();
        enqueue(ctx, ctx->slots[0], pk, cs, z_host, z_dev, r, s_, true, ctx->checked ? 0 : -1);
        finish(ctx, ctx->slots[0], pk, out, tm);
        raise_unsatisfied(ctx, 1, cs);
    }
    // ---- `count` proofs, ctx->nslots in flight: while the GPU works on proof i the host finishes proof i-(nslots-1) and enqueues proof
    // i+1, so the latency-bound tail of one proof (the H fold) overlaps the MSMs of the next.  `enq(i, slot)` enqueues proof i,
    // `fin(j, slot, timings)` finishes proof j; in checked mode the call ends in ZKHIP_ERR_UNSATISFIED if a proof failed.
    template <class Enq, class Fin>
    static void run_batch(zkhip_ctx* ctx, const zkhip_r1cs* cs, u32 count, zkhip_timings* tm, Enq enq, Fin fin) {
        zkhip_timings acc, one;
        memset(&acc, 0, sizeof(acc));
        const auto t0 = std::chrono::steady_clock::now();
        ctx->unsat.clear();
        try {
            const u32 NS = (u32)ctx->nslots;   // proofs in flight
            for (u32 i = 0; i < count + NS - 1; ++i) {
                if (i < count) enq(i, ctx->slots[i % NS]);
                if (i >= NS - 1 && i - (NS - 1) < count) {
                    const u32 j = i - (NS - 1);
                    fin(j, ctx->slots[j % NS], &one);
                    float* a = (float*)&acc; const float* b = (const float*)&one;
                    for (size_t k = 0; k < sizeof(acc) / sizeof(float); ++k) a[k] += b[k];
                }
            }
        } catch (...) {
            for (auto& sl : ctx->slots) sl.busy = false;   // let the queues drain; the context stays usable
            dev_sync_all();
            throw;
        }
        if (tm) {
            *tm = acc;
            tm->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        raise_unsatisfied(ctx, count, cs);
    }
    // z_host: count x m x 32 B, or nullptr with z_dev[i] = device pointers of resident assignments; rs: count x (r | s)
    static void prove_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* cs, u32 count, const uint8_t* z_host, void* const* z_dev,
                            const uint8_t* rs, uint8_t* proofs_out, zkhip_timings* tm) {
        run_batch(ctx, cs, count, tm,
                  [&](u32 i, ProofSlot& sl) {
                      enqueue(ctx, sl, pk, cs, z_host ? z_host + (size_t)i * pk->m * 32 : nullptr, z_host ? nullptr : z_dev[i], rs + (size_t)i * 64,
                              rs + (size_t)i * 64 + 32, false, ctx->checked ? (int)i : -1);
                  },
                  [&](u32 j, ProofSlot& sl, zkhip_timings* one) { finish(ctx, sl, pk, proofs_out + (size_t)j * PROOF_BYTES, one); });
    }
    static void assignment_upload(zkhip_ctx* ctx, zkhip_assignment* a, const uint8_t* z) {
        DBuf flag;
        upload_z(ctx, a->scalars, a->m, a->m + 2, z, flag);
        u32 verdict = 0;
        dev_d2h(&verdict, flag.p, 4, ctx->stream);
        stream_sync(ctx->stream);
        require_canonical(verdict);
    }
    // the same resident assignment from its packed form (validated on the host: zkhip_api.hip): one copy of the packed bytes, one
    // launch that widens them and tests the 32-byte values against r, the same verdict word
    static void assignment_upload_packed(zkhip_ctx* ctx, zkhip_assignment* a, const uint8_t* packed, size_t len, u64 tags_off, u64 index_off,
                                         u64 payload_off) {
        Stream s = ctx->stream;
        DBuf flag;
        unpack_z(ctx, a->scalars, a->m, a->m + 2, PackedZ{packed, len, tags_off, index_off, payload_off}, flag);
        u32 verdict = 0;
        dev_d2h(&verdict, flag.p, 4, s);
        stream_sync(s);
        require_canonical(verdict);
    }

    // the same resident assignment from the bytes of a witness file (framing checked on the host: zkhip_api.hip), waiting for its verdict;
    // `head` (l x 32 B, may be null) receives the head of z, where the public inputs are
    static void assignment_upload_witness(zkhip_ctx* ctx, zkhip_assignment* a, const WitnessZ& wz, uint8_t* head) {
        Stream s = ctx->stream;
        DBuf flag;
        ingest_z(ctx, a->scalars, a->m, a->m + 2, wz, flag);
        u32 verdict[4] = {0, 0, 0, 0};
        dev_d2h(verdict, flag.p, 16, s);
        if (head) dev_d2h(head, a->scalars.p, wz.plan->host->l * 32, s);
        stream_sync(s);
        require_verdict(verdict[0], verdict[2], wz.plan->host.get());
    }

    // ---- witnesses computed on the device (wexec.cuh): `count` instances of the plan's program, a chunk at a time, on the context's
    // exec stream and in its exec buffers — no proof slot, no other stream.  Per chunk: the arguments in, k_exec_program (or, with
    // ZKHIP_TUNE_EXEC_WIDE, the plan's levels as launches of k_exec_level / k_exec_levels_run), the verdict
    // words back (the host makes a resident assignment for every instance that ran through), then the gathers and the copies out.
    // made[i]: the assignment of instance i, or null.  Returns the number of instances that failed a check.
    static u64 compute_witness(zkhip_ctx* ctx, const zkhip_xplan* plan, u32 count, const uint8_t* args, std::vector<std::unique_ptr<zkhip_assignment>>* made,
                               uint8_t* witness_out, u64 witness_cap_each, uint8_t* inputs_out, u64 inputs_cap_each, int32_t* status, u64* first_statement,
                               u64* first_row) {
        const XPlanHost& h = *plan->host;
        Stream s = ctx_exec_stream(ctx);
        const u64 m = h.l + h.w, n_in = h.input_cols.size(), entries = h.file_ids.size(), file_bytes = h.file_bytes();
        const u64 per_instance = h.store_bytes_per_instance() + h.n_args * 32 + 4 + sizeof(void*) + (witness_out ? file_bytes : 0) + (inputs_out ? n_in * 32 : 0);
        const u64 chunk = std::min<u64>(ctx->exec_chunk > 0 ? (u64)ctx->exec_chunk : exec_chunk_default(ctx, per_instance), count);
        ctx->xstore.ensure(h.slots * chunk * sizeof(Fr));
        ctx->xargs.ensure(std::max<u64>(h.n_args, 1) * chunk * 32);
        ctx->xverdict.ensure(chunk * 4);
        if (made) ctx->xptrs.ensure(chunk * sizeof(void*));
        if (witness_out) ctx->xfile.ensure(chunk * file_bytes);
        if (inputs_out) ctx->xinputs.ensure(std::max<u64>(n_in, 1) * chunk * 32);
        std::vector<u32> verdict(chunk);
        std::vector<void*> ptrs(chunk);
        std::vector<uint8_t> tmp;
        u64 n_failed = 0;
        // the route (read at each call): one work-item per instance, or the plan's levels cut into launches at wide_min
        const bool wide = ctx->exec_wide;
        const u32 wide_min = (u32)(ctx->exec_wide_min > 0 ? ctx->exec_wide_min : EXEC_WIDE_MIN_DEFAULT);
        const u32 n_levels = h.level_start.empty() ? 0 : (u32)h.level_start.size() - 1;
        u64 launches = 1;
        if (wide) {
            launches = 0;
            bool in_run = false;
            for (u32 lv = 0; lv < n_levels; ++lv) {
                const bool narrow = h.level_start[lv + 1] - h.level_start[lv] < wide_min;
                launches += !narrow || !in_run;
                in_run = narrow;
            }
        }
        ctx->exec_last[0] = wide ? 2 : 1;
        ctx->exec_last[1] = (count + chunk - 1) / chunk;
        ctx->exec_last[2] = launches;
        ctx->exec_last[3] = wide_min;
        for (u64 c0 = 0; c0 < count; c0 += chunk) {
            const u32 c = (u32)std::min<u64>(chunk, count - c0);
            const dim3 waves(blocks_for(c, WX_BLOCK));
            if (h.n_args) dev_h2d(ctx->xargs.p, args + c0 * h.n_args * 32, (size_t)c * h.n_args * 32, s);
            if (!wide) {
                ZK_LAUNCH((k_exec_program<Fr>), waves, dim3(WX_BLOCK), 0, s, ptr<u32>(plan->code), ptr<u32>(plan->pool), ptr<uint8_t>(ctx->xargs), (u32)h.n_args, c, chunk,
                          ptr<Fr>(ctx->xstore), ptr<u32>(ctx->xverdict));
            } else {
                // the levels in ascending order: a level of wide_min instructions or more is a launch of its own over the whole
                // device, every maximal run of narrower ones a launch of one workgroup per instance; the stream orders the launches
                ZK_LAUNCH((k_exec_begin<Fr>), waves, dim3(WX_BLOCK), 0, s, c, ptr<Fr>(ctx->xstore), ptr<u32>(ctx->xverdict));
                for (u32 lv = 0; lv < n_levels;) {
                    const u32 first = h.level_start[lv], width = h.level_start[lv + 1] - first;
                    if (width >= wide_min) {
                        ZK_LAUNCH((k_exec_level<Fr>), dim3(blocks_for(width, WX_BLOCK), std::min<u32>(c, 65535)), dim3(WX_BLOCK), 0, s, ptr<u32>(plan->code), ptr<u32>(plan->pool),
                                  ptr<u32>(plan->sched), first, width, ptr<uint8_t>(ctx->xargs), (u32)h.n_args, c, chunk, ptr<Fr>(ctx->xstore), ptr<u32>(ctx->xverdict));
                        ++lv;
                        continue;
                    }
                    u32 end = lv + 1;
                    while (end < n_levels && h.level_start[end + 1] - h.level_start[end] < wide_min) ++end;
                    ZK_LAUNCH((k_exec_levels_run<Fr>), dim3(c), dim3(WX_RUN_BLOCK), 0, s, ptr<u32>(plan->code), ptr<u32>(plan->pool), ptr<u32>(plan->sched),
                              ptr<u32>(plan->level_start), lv, end, ptr<uint8_t>(ctx->xargs), (u32)h.n_args, chunk, ptr<Fr>(ctx->xstore), ptr<u32>(ctx->xverdict));
                    lv = end;
                }
            }
            dev_d2h(verdict.data(), ctx->xverdict.p, (size_t)c * 4, s);
            stream_sync(s);
            for (u32 i = 0; i < c; ++i) {
                const bool ok = verdict[i] == WX_RAN_THROUGH;
                n_failed += !ok;
                status[c0 + i] = ok ? ZKHIP_OK : ZKHIP_ERR_UNSATISFIED;
                const u64 st = ok ? ~(u64)0 : verdict[i];
                if (first_statement) first_statement[c0 + i] = st;
                if (first_row) first_row[c0 + i] = ok || st >= h.row_of.size() || h.row_of[st] == XPLAN_NO_ROW ? ~(u64)0 : h.row_of[st];
                ptrs[i] = nullptr;
                if (made && ok) {
                    std::unique_ptr<zkhip_assignment> a(new zkhip_assignment());
                    a->curve = h.curve; a->ctx = ctx; a->m = m;
                    a->scalars.ensure((m + 2) * 32);
                    ptrs[i] = a->scalars.p;
                    (*made)[c0 + i] = std::move(a);
                }
            }
            if (made) {
                dev_h2d(ctx->xptrs.p, ptrs.data(), (size_t)c * sizeof(void*), s);
                ZK_LAUNCH((k_exec_gather<Fr>), dim3((unsigned)(m + 2), waves.x), dim3(WX_BLOCK), 0, s, ptr<Fr>(ctx->xstore), chunk, c, (const u32*)nullptr, m,
                          ptr<u32>(ctx->xverdict), (Fr* const*)ctx->xptrs.p, (Fr*)nullptr, (u64)0, 1, 2u);
            }
            if (witness_out) {
                ZK_LAUNCH((k_exec_witness_file<Fr>), dim3((unsigned)entries, waves.x), dim3(WX_BLOCK), 0, s, ptr<Fr>(ctx->xstore), chunk, c,
                          (const long long*)plan->file_ids.p, ptr<u32>(plan->file_slots), entries, ptr<u32>(ctx->xverdict), ptr<uint8_t>(ctx->xfile), file_bytes);
                if (witness_cap_each == file_bytes) {
                    dev_d2h(witness_out + c0 * file_bytes, ctx->xfile.p, (size_t)c * file_bytes, s);
                } else {
                    tmp.resize((size_t)c * file_bytes);
                    dev_d2h(tmp.data(), ctx->xfile.p, tmp.size(), s);
                    stream_sync(s);
                    for (u32 i = 0; i < c; ++i) memcpy(witness_out + (c0 + i) * witness_cap_each, tmp.data() + (size_t)i * file_bytes, file_bytes);
                }
            }
            if (inputs_out && n_in) {
                ZK_LAUNCH((k_exec_gather<Fr>), dim3((unsigned)n_in, waves.x), dim3(WX_BLOCK), 0, s, ptr<Fr>(ctx->xstore), chunk, c, ptr<u32>(plan->input_cols), n_in,
                          ptr<u32>(ctx->xverdict), (Fr* const*)nullptr, ptr<Fr>(ctx->xinputs), n_in, 0, 0u);
                if (inputs_cap_each == n_in) {
                    dev_d2h(inputs_out + c0 * n_in * 32, ctx->xinputs.p, (size_t)c * n_in * 32, s);
                } else {
                    tmp.resize((size_t)c * n_in * 32);
                    dev_d2h(tmp.data(), ctx->xinputs.p, tmp.size(), s);
                    stream_sync(s);
                    for (u32 i = 0; i < c; ++i) memcpy(inputs_out + (c0 + i) * inputs_cap_each * 32, tmp.data() + (size_t)i * n_in * 32, n_in * 32);
                }
            }
            stream_sync(s);      // (the next chunk writes the same store; the assignments are complete when the call returns)
        }
        return n_failed;
    }

    // generic MSM primitive (bases in ark encoding)
    template <class F, int NC>
    static void msm_api(zkhip_ctx* ctx, u64 n, const uint8_t* bases, const uint8_t* scalars, uint8_t* out) {
        constexpr int PB = FQB * NC;
        memset(out, 0, PB + 1);
        if (n == 0) { out[PB] = 1; return; }
        require(n < ((u64)1 << 31), ZKHIP_ERR_BAD_ARG, "too many points");
        Stream s = ctx->stream;
        std::vector<uint8_t> host(n * PB);
        for (u64 i = 0; i < n; ++i) decode_point<FQB, NC>(bases + i * PB, &host[i * PB]);
        DBuf d_bases, d_ws;
        d_bases.ensure(host.size());
        dev_h2d(d_bases.p, host.data(), host.size(), s);
        ZK_LAUNCH((k_to_mont<Fq>), dim3(blocks_for(n * NC, 256)), dim3(256), 0, s, ptr<Fq>(d_bases), ptr<Fq>(d_bases), n * NC);
        ctx->cur->scalars.ensure(n * 32);
        dev_h2d(ctx->cur->scalars.p, scalars, n * 32, s);
        // ad-hoc bases: no table of window multiples (building one costs ~15x the MSM itself), one bucket set per window
        const MsmShape sh = msm_shape(&ctx->msm,n, Fr::Params::BITS, false);
        d_ws.ensure((size_t)sh.nsums() * sizeof(Xyzz<F>));
        // the packed bases are written on the main stream BEFORE the sort records `ready` there: the lane stream waits on
        // that event only, so everything the accumulation reads must precede it on the main stream
        DBuf d_packed;
        d_packed.ensure(n * packed_point_bytes<F>());
#ifdef ZK_TEST_MSM_RACE   // round 2's ordering, kept ONLY to show that tests/test_stream_jitter.py catches it (never built into libzkhip.so)
        msm_prepare(ctx, s, ctx->cur->sorts[0], ptr<u32>(ctx->cur->scalars), sh, 0);
        points_to_packed<F>(ctx, ptr<Aff<F>>(d_bases), d_packed.p, n);
#else
        points_to_packed<F>(ctx, ptr<Aff<F>>(d_bases), d_packed.p, n);
        msm_prepare(ctx, s, ctx->cur->sorts[0], ptr<u32>(ctx->cur->scalars), sh, 0);
#endif
        msm_run<F>(ctx, ctx->cur->lanes[0], ctx->cur->sorts[0], d_packed.p, sh, ptr<Xyzz<F>>(d_ws), nullptr, nullptr);
        stream_wait_event(s, ctx->cur->lanes[0].done);
        std::vector<Xyzz<F>> ws(sh.nsums());
        dev_d2h(ws.data(), d_ws.p, ws.size() * sizeof(Xyzz<F>), s);
        stream_sync(s);
        Xyzz<F> res = msm_combine(ws.data(), sh);
        if (res.is_inf()) { out[PB] = 1; return; }
        Aff<F> a = xyzz_to_affine(res);
        uint8_t tmp[sizeof(Aff<F>)];
        Aff<F> canon = from_mont_point(a);
        memcpy(tmp, &canon, sizeof(canon));
        memcpy(out, tmp, PB);
    }
    static Aff<Fq> from_mont_point(const Aff<Fq>& p) { return {fe_from_mont(p.x), fe_from_mont(p.y)}; }
    static Aff<Fq2> from_mont_point(const Aff<Fq2>& p) { return {fe_from_mont(p.x), fe_from_mont(p.y)}; }

    static void witness_map_api(zkhip_ctx* ctx, const zkhip_r1cs* cs, const uint8_t* z, uint8_t* h_out) {
        ctx->ws = ctx->stream;
        NttPlan<C>* pl = get_plan<C>(ctx, cs->logN);
        const u64 m = cs->l + cs->w;
        uint8_t zero[32] = {0};
        upload_z(ctx, ctx->cur->scalars, m, m + 2, z, ctx->cur->zflag);
        stage_scalars(ctx, pl, ctx->cur->scalars.p, m, zero, zero);
        witness_map(ctx, cs, pl);
        ctx->cur->vb.ensure(pl->N * sizeof(Fr));
        ZK_LAUNCH((k_sigma_permute<Fr>), dim3(blocks_for(pl->N, 256)), dim3(256), 0, ctx->stream, ptr<Fr>(ctx->cur->va), ptr<Fr>(ctx->cur->vb), pl->N,
                  pl->N1, pl->N2, 1, pl->N3);
        dev_d2h(h_out, ctx->cur->vb.p, pl->N * 32, ctx->stream);
        stream_sync(ctx->stream);
    }

    // The witness map of `witness_map` (unbound: six transforms) in four steps around three all-to-alls; a, b, c in the slot's va,
    // on ctx->ws.  Step 0 ends with a, b, c packed behind their inverse transforms' outer pass; 1: their ranges (a, b leave with
    // s_coset, c with s_cexit as canonical integers), the coset transform's passes over the range, a and b packed; 2: its outer pass,
    // the quotient on the strip, the last transform's outer pass, one vector packed; 3: its range, canonical, minus c's share — the
    // member's h coefficients are positions [k N/G, (k+1) N/G) of va, sigma order.  (Every step is one member's part; the caller runs a
    // step on every member before the next on any: ntt_host.cuh, shard_ntt_begin.)
    static void shard_witness_map(zkhip_ctx* ctx, const zkhip_r1cs* cs, NttPlan<C>* pl, u32 G, u32 k, int step, zkhip_ctx* const* members, bool check = false) {
        require(Tr::shard_ok(pl, G), ZKHIP_ERR_BAD_ARG, "internal: this transform does not shard");
        const ShardGeom g = ntt_shard_geom(pl->N1, pl->Nb, G);
        Stream s = ctx->ws;
        const u64 N = pl->N;
        Fr *a = ptr<Fr>(ctx->cur->va), *b = a + N, *c = b + N;
        const bool three = pl->log3 > 0;
        if (step == 0) {
            ctx->cur->va.ensure(3 * N * sizeof(Fr));
            a = ptr<Fr>(ctx->cur->va); b = a + N; c = b + N;
            Tr::shard_state(ctx, g, 3);
            matvec(ctx, cs, ptr<Fr>(ctx->cur->zmont), a, b, c, cs->n, cs->l, N, 3);
            if (check) enqueue_check(*ctx->cur, a, b, c, cs->n, s);
            event_record(ctx->cur->ntt_b, s);
            Tr::ntt_cols(ctx, pl, g, k, a, true, ptr<Fr>(pl->tw_inv), 3, N);
            Tr::shard_pack(ctx, g, k, a, 3, N, true);
        } else if (step == 1) {
            Tr::shard_fetch(ctx, g, k, a, 3, N, false, members);
            if (three) Tr::ntt_mid(ctx, pl, g, k, a, true, ptr<Fr>(pl->tw2_inv), pl->Nb - 1, 3, N);
            Tr::ntt_rows(ctx, pl, g, k, a, true, ptr<Fr>(pl->s_coset), 2, N);
            Tr::ntt_rows(ctx, pl, g, k, c, true, ptr<Fr>(pl->s_cexit), 1, 0, 1);
            if (three) {
                Tr::ntt_rows(ctx, pl, g, k, a, false, ptr<Fr>(pl->tw2_fwd), 2, N, 0, nullptr, pl->Nb - 1);
                Tr::ntt_mid(ctx, pl, g, k, a, false, ptr<Fr>(pl->tw_fwd), ~(u64)0, 2, N);
            } else {
                Tr::ntt_rows(ctx, pl, g, k, a, false, ptr<Fr>(pl->tw_fwd), 2, N);
            }
            Tr::shard_pack(ctx, g, k, a, 2, N, false);
        } else if (step == 2) {
            Tr::shard_fetch(ctx, g, k, a, 2, N, true, members);
            Tr::ntt_cols(ctx, pl, g, k, a, false, nullptr, 2, N);
            const u64 off = g.strip_origin(k);
            ZK_LAUNCH((k_quotient_strip<typename Fr::Params>), dim3(blocks_for(g.range_len(), 256)), dim3(256), 0, s, a + off, b + off, pl->zinv_rp, a + off, pl->N1,
                      ilog2_floor(g.W), pl->Nb);
            Tr::ntt_cols(ctx, pl, g, k, a, true, ptr<Fr>(pl->tw_inv), 1, 0);
            Tr::shard_pack(ctx, g, k, a, 1, 0, true);
        } else {
            Tr::shard_fetch(ctx, g, k, a, 1, 0, false, members);
            if (three) Tr::ntt_mid(ctx, pl, g, k, a, true, ptr<Fr>(pl->tw2_inv), pl->Nb - 1, 1, 0);
            Tr::ntt_rows(ctx, pl, g, k, a, true, ptr<Fr>(pl->s_cosetinv_canon), 1, 0, 1, c);
            event_record(ctx->cur->ntt_e, s);
        }
    }
    static int witness_map_shardable_api(zkhip_ctx* ctx, const zkhip_r1cs* cs, u32 G) { return Tr::ntt_shardable_api(ctx, (u32)cs->logN, G); }
    // zkhip_multi_witness_map: step 0 stages the assignment first, step 3 hands the member's part of h out (h_out: N x 32 B, natural order)
    static void shard_witness_map_api(zkhip_ctx* ctx, const zkhip_r1cs* cs, const uint8_t* z, uint8_t* h_out, u32 G, u32 k, int step, zkhip_ctx* const* members) {
        ctx->ws = ctx->stream;
        NttPlan<C>* pl = get_plan<C>(ctx, cs->logN);
        if (step == 0) {
            const u64 m = cs->l + cs->w;
            uint8_t zero[32] = {0};
            upload_z(ctx, ctx->cur->scalars, m, m + 2, z, ctx->cur->zflag);
            stage_scalars(ctx, pl, ctx->cur->scalars.p, m, zero, zero);
        }
        shard_witness_map(ctx, cs, pl, G, k, step, members);
        if (step == 3) Tr::range_out(ctx, pl, ntt_shard_geom(pl->N1, pl->Nb, G), k, ptr<Fr>(ctx->cur->va), 0, Fr::one(), Fr::one(), h_out);
    }

    // zkhip_field_op: count x (a op b) over elements F, canonical integers in and out, in workgroups of T; `launch` runs the kernel
    // of the field's form on the two Montgomery vectors, result into the first (field_op_dispatch names the six)
    template <class F, class Launch>
    static void field_op_api(zkhip_ctx* ctx, u64 count, unsigned T, const uint8_t* a, const uint8_t* b, uint8_t* out, Launch launch) {
        Stream s = ctx->stream;
        const size_t bytes = count * sizeof(F);
        ctx->cur->va.ensure(bytes); ctx->cur->vb.ensure(bytes);
        dev_h2d(ctx->cur->va.p, a, bytes, s);
        dev_h2d(ctx->cur->vb.p, b, bytes, s);
        const unsigned B = blocks_for(count, T);
        ZK_LAUNCH((k_to_mont<F>), dim3(B), dim3(T), 0, s, ptr<F>(ctx->cur->va), ptr<F>(ctx->cur->va), count);
        ZK_LAUNCH((k_to_mont<F>), dim3(B), dim3(T), 0, s, ptr<F>(ctx->cur->vb), ptr<F>(ctx->cur->vb), count);
        launch(dim3(B), dim3(T), s, ptr<F>(ctx->cur->va), ptr<F>(ctx->cur->vb));
        ZK_LAUNCH((k_from_mont<F>), dim3(B), dim3(T), 0, s, ptr<F>(ctx->cur->va), ptr<F>(ctx->cur->va), count);
        dev_d2h(out, ctx->cur->va.p, bytes, s);
        stream_sync(s);
    }

    static void r1cs_load(zkhip_ctx* ctx, zkhip_r1cs* cs, const u64* const rp[3], const u32* const col[3], const uint8_t* const val[3]) {
        Stream s = ctx->stream;
        std::vector<u64> long_rows, huge_rows;
        const u64 huge_min = env_int("ZKHIP_MATVEC_HUGE", 0, 1, 1) ? (u64)MATVEC_HUGE : ~(u64)0;     // (0: every long row to k_matvec_long, for A/B runs)
        for (int k = 0; k < 3; ++k) {
            const u64 nnz = rp[k][cs->n];
            require(rp[k][0] == 0, ZKHIP_ERR_BAD_ARG, "rowptr[0] must be 0");
            for (u64 i = 0; i < cs->n; ++i) require(rp[k][i] <= rp[k][i + 1], ZKHIP_ERR_BAD_ARG, "rowptr not monotone");
            cs->nnz_short[k] = nnz;
            for (u64 i = 0; i < cs->n; ++i)
                if (rp[k][i + 1] - rp[k][i] > MATVEC_LONG) {
                    (rp[k][i + 1] - rp[k][i] > huge_min ? huge_rows : long_rows).push_back((u64)k << 32 | i);
                    cs->nnz_short[k] -= rp[k][i + 1] - rp[k][i];
                }
            for (u64 q = 0; q < nnz; ++q) require(col[k][q] < cs->l + cs->w, ZKHIP_ERR_BAD_ARG, "column index out of range");
            cs->nnz[k] = nnz;
            cs->rp[k].ensure((cs->n + 1) * 8);
            cs->col[k].ensure(std::max<u64>(nnz, 1) * 4);
            cs->val[k].ensure(std::max<u64>(nnz, 1) * 32);
            dev_h2d(cs->rp[k].p, rp[k], (cs->n + 1) * 8, s);
            if (nnz) {
                dev_h2d(cs->col[k].p, col[k], nnz * 4, s);
                dev_h2d(cs->val[k].p, val[k], nnz * 32, s);
                ZK_LAUNCH((k_to_mont<Fr>), dim3(blocks_for(nnz, 256)), dim3(256), 0, s, ptr<Fr>(cs->val[k]), ptr<Fr>(cs->val[k]), nnz);
            }
        }
        cs->n_huge = huge_rows.size();
        long_rows.insert(long_rows.begin(), huge_rows.begin(), huge_rows.end());     // the huge rows first
        cs->n_long = long_rows.size();
        if (cs->n_long) {
            cs->long_rows.ensure(cs->n_long * 8);
            dev_h2d(cs->long_rows.p, long_rows.data(), cs->n_long * 8, s);
        }
        stream_sync(s);
    }
};

}  // namespace zk

#include "setup.cuh"
#include "gm17.cuh"
#include "pairing.cuh"

// ------------------------------------------------------------------ per-curve entry points
namespace zk {
struct CurveOps {
    void (*pk_load)(zkhip_ctx*, int scheme, const uint8_t*, size_t, zkhip_pk*);
    u64 (*pk_export_size)(const zkhip_pk*);
    void (*pk_export)(zkhip_pk*, uint8_t*, u64);
    void (*pk_import)(zkhip_ctx*, const uint8_t*, size_t, zkhip_pk*);
    void (*pk_bind)(zkhip_ctx*, zkhip_pk*, const zkhip_r1cs*);
    void (*pk_bind_check)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*);
    void (*pk_unbind)(zkhip_pk*);
    void (*bound_level0_from_file)(zkhip_ctx*, int scheme, const zkhip_r1cs*, const uint8_t*, size_t, std::vector<uint8_t>&, std::vector<uint8_t>&, u64 fp[2]);
    void (*install_bound_ranges)(zkhip_ctx*, zkhip_pk*, const zkhip_r1cs*, const uint8_t*, size_t, const uint8_t*, size_t, const u64 fp[2]);
    void (*r1cs_fingerprint)(zkhip_ctx*, const zkhip_r1cs*, u64 fp[2]);
    bool (*can_split)(const zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*);
    void (*split_begin)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const void*, const uint8_t*, const uint8_t*, int half);
    const void* (*split_half_ptr)(zkhip_ctx*, const zkhip_pk*, int half);
    void (*split_fetch)(zkhip_ctx*, const zkhip_pk*, const void*, int, Event);
    void (*split_fetch_host)(zkhip_ctx*, const zkhip_pk*, const uint8_t*);
    void (*split_half_out)(zkhip_ctx*, const zkhip_pk*, uint8_t*);
    void (*split_end_partial)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, uint8_t*, zkhip_timings*);
    void (*split_end_device_sums)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const void**, size_t*, const void**, size_t*, zkhip_timings*);
    void (*r1cs_load)(zkhip_ctx*, zkhip_r1cs*, const u64* const rp[3], const u32* const col[3], const uint8_t* const val[3]);
    void (*prove)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t* z_host, const void* z_dev, const uint8_t*, const uint8_t*, uint8_t*,
                  zkhip_timings*);
    void (*prove_batch)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, u32, const uint8_t*, void* const*, const uint8_t*, uint8_t*, zkhip_timings*);
    void (*prove_partial)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const void*, const uint8_t*, const uint8_t*, uint8_t*,
                          zkhip_timings*);
    void (*combine)(const zkhip_pk*, u32, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*);
    size_t partial_bytes;
    void (*prove_device_sums)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const uint8_t*, const uint8_t*, const void**, size_t*,
                              const void**, size_t*, zkhip_timings*);
    void (*gm17_prove_device_sums)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const uint8_t*, const void**, size_t*, const void**,
                                   size_t*, zkhip_timings*);
    void (*record_from_sums)(zkhip_ctx*, const zkhip_pk*, const uint8_t*, const uint8_t*, uint8_t*);
    void (*assignment_upload)(zkhip_ctx*, zkhip_assignment*, const uint8_t*);
    void (*assignment_upload_packed)(zkhip_ctx*, zkhip_assignment*, const uint8_t*, size_t, u64, u64, u64);
    void (*assignment_upload_witness)(zkhip_ctx*, zkhip_assignment*, const WitnessZ&, uint8_t* head);
    u64 (*compute_witness)(zkhip_ctx*, const zkhip_xplan*, u32, const uint8_t*, std::vector<std::unique_ptr<zkhip_assignment>>*, uint8_t*, u64, uint8_t*, u64,
                           int32_t*, u64*, u64*);
    void (*r1cs_check)(zkhip_ctx*, const zkhip_r1cs*, const uint8_t*, const void*, u64 out[2]);
    void (*ntt)(zkhip_ctx*, u32, int, uint8_t*);
    void (*witness_map)(zkhip_ctx*, const zkhip_r1cs*, const uint8_t*, uint8_t*);
    // sharded across the members of a zkhip_multi (ntt_shard.h): member k of G, step by step
    int (*ntt_shardable)(zkhip_ctx*, u32 log_n, u32 G);       // the plan's split, or -1
    void (*shard_ntt_begin)(zkhip_ctx*, u32 G, u32 k, u32 log_n, int dir, const uint8_t*);
    void (*shard_ntt_end)(zkhip_ctx*, u32 G, u32 k, u32 log_n, int dir, uint8_t*, zkhip_ctx* const* members);
    int (*witness_map_shardable)(zkhip_ctx*, const zkhip_r1cs*, u32 G);
    void (*shard_witness_map)(zkhip_ctx*, const zkhip_r1cs*, const uint8_t* z, uint8_t* h_out, u32 G, u32 k, int step, zkhip_ctx* const* members);
    int (*can_shard)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, u32 G, u32 k);
    void (*shard_begin)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const uint8_t*, const uint8_t*, u32 G, u32 k);
    void (*shard_step)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, u32 G, u32 k, int step, zkhip_ctx* const* members);
    void (*shard_end_partial)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, uint8_t*, zkhip_timings*);
    void (*shard_end_device_sums)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const void**, size_t*, const void**, size_t*, zkhip_timings*);
    void (*msm_g1)(zkhip_ctx*, u64, const uint8_t*, const uint8_t*, uint8_t*);
    void (*msm_g2)(zkhip_ctx*, u64, const uint8_t*, const uint8_t*, uint8_t*);
    void (*field_op)(zkhip_ctx*, int field, int op, u64, const uint8_t*, const uint8_t*, uint8_t*);
    void (*group_op)(zkhip_ctx*, int group, int form, int op, u64, const u32*, const u32*, const u32*, const uint8_t*, u32*);
    void (*setup)(zkhip_ctx*, const zkhip_r1cs*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, u64);
    // the pairing check on the device (pairing.cuh)
    void (*pairing_products)(zkhip_ctx*, u64 count, u32 pairs_per_item, const uint8_t* g1, const uint8_t* g2, uint8_t* ok_out);
    void (*tower_op)(zkhip_ctx*, int op, u64 count, const u32*, const u32*, u32*);
    void (*vk_load)(zkhip_ctx*, int scheme, const uint8_t*, size_t, zkhip_vk*);
    void (*verify)(zkhip_ctx*, const zkhip_vk*, u64 count, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out);
    u32 tower_limbs;          // limbs of one Fq element in the unsaturated form
    // GM17 (gm17.cuh)
    void (*gm17_prove)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const void*, const uint8_t*, uint8_t*, zkhip_timings*);
    void (*gm17_prove_batch)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, u32, const uint8_t*, void* const*, const uint8_t*, uint8_t*,
                             zkhip_timings*);
    void (*gm17_setup)(zkhip_ctx*, const zkhip_r1cs*, const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, u64);
    u64 (*gm17_key_bytes)(u64, u64, u64);
    void (*gm17_prove_partial)(zkhip_ctx*, const zkhip_pk*, const zkhip_r1cs*, const uint8_t*, const void*, const uint8_t*, uint8_t*, zkhip_timings*);
    void (*gm17_combine)(const zkhip_pk*, u32, const uint8_t*, const uint8_t*, uint8_t*);
    // the proof queue (gm17.cuh QueueOps): either scheme, the key's
    void (*queue_check)(const zkhip_pk*, const zkhip_r1cs*);
    void (*queue_enqueue)(zkhip_ctx*, ProofSlot&, const zkhip_pk*, const zkhip_r1cs*, const uint8_t* z_host, const void* z_dev, const PackedZ*, const WitnessZ*,
                          const uint8_t* rnd, bool checked);
    void (*queue_finish)(zkhip_ctx*, ProofSlot&, const zkhip_pk*, uint8_t*, zkhip_timings*);
};
// fields of zkhip_field_op: 0 Fr, 1 Fq, 2 Fq2 in the saturated form; 3 Fq2, 4 Fr, 5 Fq in the unsaturated limbs of the MSM kernels
// and the transform passes (k_field_op_fq2, k_field_op_unsat)
template <class C>
static void field_op_dispatch(zkhip_ctx* ctx, int field, int op, u64 count, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    typedef typename C::Fr Fr;
    typedef typename C::Fq Fq;
    typedef typename C::Fq2 Fq2;
    typedef Prover<C> P;
    if (field == 0) P::template field_op_api<Fr>(ctx, count, 256, a, b, out, [&](dim3 g, dim3 t, Stream s, Fr* x, Fr* y) { ZK_LAUNCH((k_field_op<Fr>), g, t, 0, s, x, y, x, count, op); });
    else if (field == 1) P::template field_op_api<Fq>(ctx, count, 256, a, b, out, [&](dim3 g, dim3 t, Stream s, Fq* x, Fq* y) { ZK_LAUNCH((k_field_op<Fq>), g, t, 0, s, x, y, x, count, op); });
    else if (field == 2) P::template field_op_api<Fq2>(ctx, count, 64, a, b, out, [&](dim3 g, dim3 t, Stream s, Fq2* x, Fq2* y) { ZK_LAUNCH((k_field_op_fq2<typename Fq2::Params, false>), g, t, 0, s, x, y, x, count, op); });
    else if (field == 3) P::template field_op_api<Fq2>(ctx, count, 64, a, b, out, [&](dim3 g, dim3 t, Stream s, Fq2* x, Fq2* y) { ZK_LAUNCH((k_field_op_fq2<typename Fq2::Params, true>), g, t, 0, s, x, y, x, count, op); });
    else if (field == 4) P::template field_op_api<Fr>(ctx, count, 64, a, b, out, [&](dim3 g, dim3 t, Stream s, Fr* x, Fr* y) { ZK_LAUNCH((k_field_op_unsat<typename Fr::Params>), g, t, 0, s, x, y, x, count, op); });
    else P::template field_op_api<Fq>(ctx, count, 64, a, b, out, [&](dim3 g, dim3 t, Stream s, Fq* x, Fq* y) { ZK_LAUNCH((k_field_op_unsat<typename Fq::Params>), g, t, 0, s, x, y, x, count, op); });
}
template <class C>
static void group_op_dispatch(zkhip_ctx* ctx, int group, int form, int op, u64 count, const u32* a, const u32* b, const u32* k, const uint8_t* flags, u32* out) {
    if (group == 1) group_op_run<typename C::Fq>(ctx, form, op, count, a, b, k, flags, out);
    else group_op_run<typename C::Fq2>(ctx, form, op, count, a, b, k, flags, out);
}
template <class C>
static CurveOps make_curve_ops() {
    CurveOps o;
    o.pk_load = &PkLoader<C>::load_file;
    o.pk_export_size = &PkLoader<C>::export_size;
    o.pk_export = &PkLoader<C>::export_image;
    o.pk_import = &PkLoader<C>::import_image;
    o.pk_bind = &PkLoader<C>::bind;
    o.pk_bind_check = &PkLoader<C>::bind_check;
    o.pk_unbind = &PkLoader<C>::unbind;
    o.bound_level0_from_file = &PkLoader<C>::bound_level0_from_file;
    o.install_bound_ranges = &PkLoader<C>::install_bound_ranges;
    o.r1cs_fingerprint = &PkLoader<C>::r1cs_fingerprint;
    o.can_split = &Prover<C>::can_split;
    o.split_begin = &Prover<C>::split_begin;
    o.split_half_ptr = &Prover<C>::split_half_ptr;
    o.split_fetch = &Prover<C>::split_fetch;
    o.split_fetch_host = &Prover<C>::split_fetch_host;
    o.split_half_out = &Prover<C>::split_half_out;
    o.split_end_partial = &Prover<C>::split_end_partial;
    o.split_end_device_sums = &Prover<C>::split_end_device_sums;
    o.r1cs_load = &Prover<C>::r1cs_load;
    o.prove = &Prover<C>::prove;
    o.prove_batch = &Prover<C>::prove_batch;
    o.prove_partial = &Prover<C>::prove_partial;
    o.combine = &Prover<C>::combine;
    o.partial_bytes = Prover<C>::PARTIAL_BYTES;
    o.prove_device_sums = &Prover<C>::prove_device_sums;
    o.gm17_prove_device_sums = &Gm17<C>::prove_device_sums;
    o.record_from_sums = &Prover<C>::record_from_sums;
    o.assignment_upload = &Prover<C>::assignment_upload;
    o.assignment_upload_packed = &Prover<C>::assignment_upload_packed;
    o.assignment_upload_witness = &Prover<C>::assignment_upload_witness;
    o.compute_witness = &Prover<C>::compute_witness;
    o.r1cs_check = &Prover<C>::r1cs_check;
    o.ntt = &Transforms<C>::ntt_api;
    o.witness_map = &Prover<C>::witness_map_api;
    o.ntt_shardable = &Transforms<C>::ntt_shardable_api;
    o.shard_ntt_begin = &Transforms<C>::shard_ntt_begin;
    o.shard_ntt_end = &Transforms<C>::shard_ntt_end;
    o.witness_map_shardable = &Prover<C>::witness_map_shardable_api;
    o.shard_witness_map = &Prover<C>::shard_witness_map_api;
    o.can_shard = &Prover<C>::can_shard;
    o.shard_begin = &Prover<C>::shard_begin;
    o.shard_step = &Prover<C>::shard_step;
    o.shard_end_partial = &Prover<C>::shard_end_partial;
    o.shard_end_device_sums = &Prover<C>::shard_end_device_sums;
    o.msm_g1 = &Prover<C>::template msm_api<typename C::Fq, 2>;
    o.msm_g2 = &Prover<C>::template msm_api<typename C::Fq2, 4>;
    o.field_op = &field_op_dispatch<C>;
    o.group_op = &group_op_dispatch<C>;
    o.setup = &Setup<C>::run;
    o.pairing_products = &PairingDev<C>::products;
    o.tower_op = &PairingDev<C>::tower_op;
    o.vk_load = &PairingDev<C>::vk_load;
    o.verify = &PairingDev<C>::verify;
    o.tower_limbs = (u32)Fu<typename C::Fq::Params>::N;
    o.gm17_prove = &Gm17<C>::prove;
    o.gm17_prove_batch = &Gm17<C>::prove_batch;
    o.gm17_setup = &Gm17<C>::setup;
    o.gm17_key_bytes = &Gm17<C>::key_bytes;
    o.gm17_prove_partial = &Gm17<C>::prove_partial;
    o.gm17_combine = &Gm17<C>::combine;
    o.queue_check = &QueueOps<C>::check;
    o.queue_enqueue = &QueueOps<C>::enqueue;
    o.queue_finish = &QueueOps<C>::finish;
    return o;
}
const CurveOps* curve_ops_bn254();
const CurveOps* curve_ops_bls381();
const CurveOps* curve_ops_bls377();
}  // namespace zk
