// zkhip_api.hip — the C ABI of include/zkhip.h: argument checking, error mapping, per-curve dispatch.
// The drop-in boundary for `Backend<T, G16>::generate_proof` (/root/reference/zokrates_proof_systems/src/lib.rs:98-112).
#include "core.cuh"
#include "ingest.h"
#ifndef ZK_EMU
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is loaded at run time, when zkhip_multi_use_rccl asks for it
#endif

// ------------------------------------------------------------------ C ABI
static const CurveOps* ops_for(int curve) {
    if (curve == ZKHIP_CURVE_BN128) return curve_ops_bn254();
    if (curve == ZKHIP_CURVE_BLS12_381) return curve_ops_bls381();
    if (curve == ZKHIP_CURVE_BLS12_377) return curve_ops_bls377();
    throw ApiError{ZKHIP_ERR_BAD_ARG, "unknown curve id"};
}
// errors of calls that have no context (zkhip_ctx_create, zkhip_prog_*): one message per calling thread
static thread_local std::string g_create_err;

// after a failed call: let whatever was enqueued drain and mark the proof slots free, so the context stays usable
static void release_slots(zkhip_ctx* ctx) {
    // (under an open proof queue the busy slots are ITS proofs in flight, and the only calls that come this far are the ones the
    // pending rule lets through: they enqueue nothing, so there is nothing of theirs to drain)
    if (ctx->queue) return;
    bool any = false;
    for (auto& sl : ctx->slots) any = any || sl.busy;
    if (!any) return;
    dev_sync_all();
    for (auto& sl : ctx->slots) sl.busy = false;
}
// Between zkhip_prove_g16_split_begin and _end a proof is PENDING in slot 0: its vectors, sorted lists and lanes hold the head's work,
// and its tail will take the tables and the streams the head saw.  Every entry point that enqueues on the context's streams, writes
// its workspaces, or changes a key, the streams or the mode — all of them but the ones that pass `while_pending` — is refused here,
// on the host, before anything is enqueued, and the pending proof stays as it is (no release_slots: nothing of this call is in flight)
static const char* const SPLIT_PENDING_MSG =
    "a split proof is pending in this context (zkhip_prove_g16_split_begin): finish it with zkhip_prove_g16_split_end or drop it with "
    "zkhip_prove_g16_split_abort first";
static bool split_pending(const zkhip_ctx* ctx) { return ctx->slots[0].split_pending; }
// An open proof queue (zkhip_queue_open .. zkhip_queue_close) makes its context pending in the same sense, for the same reason — up to
// ctx->nslots proofs are in flight in the slots between two calls — and the same gate refuses the same calls.  The two states exclude
// each other: each one's opening call is among the calls the other refuses.
static const char* const QUEUE_OPEN_MSG =
    "a proof queue is open in this context (zkhip_queue_open): its proofs in flight own the context's buffers and streams; collect them "
    "and close it with zkhip_queue_close first";
// an abandoned or failed split proof: what is enqueued drains, the slot is free again
static void split_drop(zkhip_ctx* ctx) {
    ProofSlot& sl = ctx->slots[0];
    if (!sl.split_pending && (!sl.busy || ctx->queue)) return;      // (nothing pending; a busy slot 0 under a queue is the queue's)
    try { dev_set(ctx->device); dev_sync_all(); } catch (...) {}
    sl.busy = false;
    sl.split_pending = false;
    sl.split_pk = nullptr;
    sl.split_cs = nullptr;
    sl.half = -1;
}
template <class Fn>
static int32_t guarded(zkhip_ctx* ctx, Fn&& fn, bool while_pending = false) {
    if (ctx && !while_pending && split_pending(ctx)) {
        ctx->err = SPLIT_PENDING_MSG;
        return ZKHIP_ERR_BAD_ARG;
    }
    if (ctx && !while_pending && ctx->queue) {
        ctx->err = QUEUE_OPEN_MSG;
        return ZKHIP_ERR_BAD_ARG;
    }
    try {
        if (ctx) dev_set(ctx->device);
        fn();
        return ZKHIP_OK;
    } catch (const ApiError& e) {
        (ctx ? ctx->err : g_create_err) = e.msg;
        if (ctx) release_slots(ctx);
        return e.code;
    } catch (const DevError& e) {
        (ctx ? ctx->err : g_create_err) = e.msg;
        if (ctx) release_slots(ctx);
        return ZKHIP_ERR_DEVICE;
    } catch (const std::bad_alloc&) {
        (ctx ? ctx->err : g_create_err) = "out of host memory";
        if (ctx) release_slots(ctx);
        return ZKHIP_ERR_NOMEM;
    } catch (...) {
        (ctx ? ctx->err : g_create_err) = "unexpected internal error";
        if (ctx) release_slots(ctx);
        return ZKHIP_ERR_DEVICE;
    }
}

// The pairing checks work on a stream and in buffers of their own and touch no proof slot: an open proof queue does not refuse
// them (checking collected proofs between submits is what they are for), a pending split proof does, as it refuses every call; and
// a call that fails leaves the proofs in flight as they are (no release_slots: nothing of theirs is this call's)
template <class Fn>
static int32_t guarded_verify(zkhip_ctx* ctx, Fn&& fn) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    if (split_pending(ctx)) {
        ctx->err = SPLIT_PENDING_MSG;
        return ZKHIP_ERR_BAD_ARG;
    }
    try {
        dev_set(ctx->device);
        fn();
        return ZKHIP_OK;
    } catch (const ApiError& e) {
        ctx->err = e.msg;
        return e.code;
    } catch (const DevError& e) {
        ctx->err = e.msg;
        return ZKHIP_ERR_DEVICE;
    } catch (const std::bad_alloc&) {
        ctx->err = "out of host memory";
        return ZKHIP_ERR_NOMEM;
    } catch (...) {
        ctx->err = "unexpected internal error";
        return ZKHIP_ERR_DEVICE;
    }
}

template <class Fn>
static int32_t guarded_host(Fn&& fn) {
    try {
        fn();
        return ZKHIP_OK;
    } catch (const IngestError& e) {
        g_create_err = e.msg;
        return e.code;
    } catch (const std::bad_alloc&) {
        g_create_err = "out of host memory";
        return ZKHIP_ERR_NOMEM;
    } catch (...) {
        g_create_err = "unexpected internal error";
        return ZKHIP_ERR_PARSE;
    }
}
// whether this library has made a HIP call in this process (after which GPU_MAX_HW_QUEUES is no longer read by the runtime)
static std::atomic<bool> g_hip_touched{false};
#ifndef ZK_EMU
// one wavefront: shader cycles against the constant-rate wall clock over `ticks` wall-clock ticks (zkhip_ctx_clock_probe)
static __global__ void k_clock_probe(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long w0 = wall_clock64(), c0 = clock64();
    while (wall_clock64() - w0 < ticks) __builtin_amdgcn_s_sleep(64);
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = w1 - w0; }
}
#endif

// a proving-key file of either scheme, resident: the whole key (rank 0 of 1) or one shard
static int32_t load_key(zkhip_ctx* ctx, int32_t curve, int scheme, const uint8_t* bytes, size_t len, uint32_t rank, uint32_t world, zkhip_pk** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(bytes && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(world >= 1 && world <= 64 && rank < world, ZKHIP_ERR_BAD_ARG, "rank / world out of range (1 <= world <= 64)");
        std::unique_ptr<zkhip_pk> pk(new zkhip_pk());
        pk->curve = curve;
        pk->ctx = ctx;
        pk->rank = rank;
        pk->world = world;
        ops_for(curve)->pk_load(ctx, scheme, bytes, len, pk.get());
        *out = pk.release();
    });
}
// What zkhip_pk_bind_r1cs and zkhip_pk_bind_r1cs_shard share.  The argument checks come first and never touch the key: a call that is
// refused leaves an earlier binding (seconds of work) as it was; only a failure INSIDE the rebuild — `rebuild(ops, started)` sets
// `started` before it drops the old tables — leaves the key as loaded
template <class Fn>
static int32_t bind_key(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* r1cs, bool args_ok, Fn&& rebuild) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    bool started = false;
    const int32_t rc = guarded(ctx, [&] {
        require(pk && r1cs && args_ok, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        for (auto& sl : ctx->slots) require(!sl.busy, ZKHIP_ERR_BAD_ARG, "a proof is in flight in this context");
        const CurveOps* ops = ops_for(pk->curve);
        ops->pk_bind_check(ctx, pk, r1cs);
        rebuild(ops, started);
    });
    if (rc != ZKHIP_OK && pk && started) zkhip_pk_unbind(pk);   // whatever failed half-way: the key is as it was loaded
    return rc;
}

// ---- the proof queue (zkhip_queue_*): the tickets, and the guard of its entry points.
// The hazard is guarded(): on ANY exception it runs release_slots, which waits for the device and frees every slot — right for a call
// that owns everything in flight, wrong here, where the other slots hold other tickets.  So the queue's calls have a guard of their own
// that tells two kinds of failure apart:
//   * one call's or one proof's — a submit refused for its arguments (thrown before its first copy or launch: QueueOps, and the checks
//     in queue_submit), a collected proof whose assignment was not canonical or not satisfying (thrown by `finish` AFTER it has waited
//     for its own slot and marked it free): the code and the message go to the caller, every other slot stays as it is;
//   * the device's (DevError, and anything that is neither ZKHIP_ERR_BAD_ARG, _PARSE nor _UNSATISFIED: it may have left half a proof
//     enqueued): the queue is broken.  The error is kept, the device drained, the slots freed; every ticket still counted as in flight
//     collects with ZKHIP_ERR_DEVICE and that text, submit answers the same, zkhip_queue_close works.
static void queue_break(zkhip_queue* q, const std::string& msg) {
    q->broken = true;
    q->dev_err = msg;
    dev_sync_all();
    for (auto& sl : q->ctx->slots) sl.busy = false;
}
template <class Fn>
static int32_t queue_guarded(zkhip_queue* q, Fn&& fn) {
    zkhip_ctx* ctx = q->ctx;
    auto broke = [&](const std::string& msg, int32_t code) {
        ctx->err = msg;
        queue_break(q, msg);
        return code;
    };
    try {
        dev_set(ctx->device);
        fn();
        return ZKHIP_OK;
    } catch (const ApiError& e) {
        if (e.code != ZKHIP_ERR_BAD_ARG && e.code != ZKHIP_ERR_PARSE && e.code != ZKHIP_ERR_UNSATISFIED) return broke(e.msg, e.code);
        ctx->err = e.msg;
        return e.code;
    } catch (const DevError& e) {
        return broke(e.msg, ZKHIP_ERR_DEVICE);
    } catch (const std::bad_alloc&) {
        return broke("out of host memory", ZKHIP_ERR_NOMEM);
    } catch (...) {
        return broke("unexpected internal error", ZKHIP_ERR_DEVICE);
    }
}
// a witness file and its plan, checked on the host before anything is enqueued: the framing with the reader's messages (ZKHIP_ERR_PARSE),
// the plan against the context and — where the caller has one — the constraint system
static WitnessZ witness_source(zkhip_ctx* ctx, const zkhip_wplan* plan, const zkhip_r1cs* cs, const uint8_t* witness, size_t len) {
    require(plan && witness, ZKHIP_ERR_BAD_ARG, "null argument");
    require(plan->ctx == ctx, ZKHIP_ERR_BAD_ARG, "the witness plan belongs to another context");
    if (cs)
        require(plan->cs_uid == cs->uid, ZKHIP_ERR_BAD_ARG, "the witness plan was made for another constraint system (zkhip_wplan_create)");
    uint64_t count = 0;
    try {
        count = witness_header_validate(witness, len);
    } catch (const IngestError& e) {
        throw ApiError{e.code, e.msg};
    }
    return WitnessZ{witness, len, count, plan};
}
// what the four witness sources share: the state first (broken, full), then the source's own checks — all on the host —, then the
// proof enqueued into the slot of the next ticket exactly as a batch call enqueues its proof of that index
static int32_t queue_submit(zkhip_queue* q, const uint8_t* z, zkhip_assignment* z_resident, const uint8_t* packed, size_t len, bool is_packed, const uint8_t* rnd,
                            uint64_t* ticket, const zkhip_wplan* plan = nullptr, bool is_witness = false) {
    if (!q || !q->ctx) return ZKHIP_ERR_BAD_ARG;
    zkhip_ctx* ctx = q->ctx;
    if (q->broken) { ctx->err = q->dev_err; return ZKHIP_ERR_DEVICE; }
    if (q->next - q->head >= q->cap) {
        ctx->err = "the proof queue holds " + std::to_string(q->cap) + " proofs in flight and all are: collect one first (zkhip_queue_collect)";
        return ZKHIP_ERR_BUSY;
    }
    return queue_guarded(q, [&] {
        const zkhip_r1cs* cs = q->cs;
        require(rnd != nullptr, ZKHIP_ERR_BAD_ARG, "null argument");
        PackedZ zp{};
        WitnessZ wz{};
        if (is_witness) {
            wz = witness_source(ctx, plan, cs, packed, len);
        } else if (is_packed) {
            require(packed != nullptr, ZKHIP_ERR_BAD_ARG, "null argument");
            // the whole structure on the host, before anything is enqueued (as zkhip_assignment_upload_packed): the kernel never sees an inconsistent buffer
            PackedLayout ly;
            try {
                ly = assignment_packed_validate(packed, len);
            } catch (const IngestError& e) {
                throw ApiError{e.code, e.msg};
            }
            const std::string dims = "the packed assignment has " + std::to_string(ly.m) + " elements, the constraint system " + std::to_string(cs->l + cs->w) + " variables (l + w)";
            require(ly.m == cs->l + cs->w, ZKHIP_ERR_BAD_ARG, dims.c_str());
            require(packed_first_is_one(packed, ly), ZKHIP_ERR_BAD_ARG, Z0_NOT_ONE_MSG);
            zp = PackedZ{packed, len, ly.tags_off, ly.index_off, ly.payload_off};
        } else {
            require((z != nullptr) != (z_resident != nullptr), ZKHIP_ERR_BAD_ARG, "exactly one of z and z_resident");
            if (z_resident)
                require(z_resident->ctx == ctx && z_resident->curve == cs->curve && z_resident->m == cs->l + cs->w, ZKHIP_ERR_BAD_ARG,
                        "assignment does not match the constraint system");
        }
        ops_for(q->pk->curve)->queue_enqueue(ctx, ctx->slots[q->next % q->cap], q->pk, cs, z, z_resident ? z_resident->scalars.p : nullptr, is_packed ? &zp : nullptr,
                                             is_witness ? &wz : nullptr, rnd, q->checked);
        if (ticket) *ticket = q->next;
        ++q->next;
    });
}

extern "C" {

int32_t zkhip_init(int32_t hw_queues) {
    if (hw_queues < 0 || hw_queues > 64) { g_create_err = "hw_queues out of range (0 .. 64)"; return ZKHIP_ERR_BAD_ARG; }
    if (hw_queues == 0) return ZKHIP_OK;
#ifndef ZK_EMU
    if (g_hip_touched.load()) { g_create_err = "zkhip_init after the library's first HIP call: the runtime has read its settings already"; return ZKHIP_ERR_BAD_ARG; }
    char buf[16];
    snprintf(buf, sizeof(buf), "%d", (int)hw_queues);
    setenv("GPU_MAX_HW_QUEUES", buf, 0);      // (0: a value the process set itself stands)
#endif
    return ZKHIP_OK;
}

int32_t zkhip_device_count(void) { g_hip_touched.store(true); return dev_count(); }

int32_t zkhip_device_pci_bus_id(int32_t device, char* out, size_t cap) {
    if (!out || cap < 13) { g_create_err = "out is NULL or shorter than 13 bytes"; return ZKHIP_ERR_BAD_ARG; }
    out[0] = 0;
    return guarded(nullptr, [&] {
        require(device >= 0 && device < dev_count(), ZKHIP_ERR_BAD_ARG, "device index out of range");
        dev_pci_bus_id(device, out, cap);
    });
}

int32_t zkhip_ctx_create(int32_t device, zkhip_ctx** out) {
    if (!out) { g_create_err = "out is NULL"; return ZKHIP_ERR_BAD_ARG; }
    *out = nullptr;
    g_hip_touched.store(true);
    return guarded(nullptr, [&] {
        // ZKHIP_INIT_PROFILE=1: where the start of a process goes (stderr; a one-proof CLI run is mostly this)
        const bool prof = getenv("ZKHIP_INIT_PROFILE") != nullptr;
        auto t_last = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (!prof) return;
            const auto t = std::chrono::steady_clock::now();
            fprintf(stderr, "[zkhip init] %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
            t_last = t;
        };
        const int n = dev_count();
        lap("runtime start (device count)");
        require(n > 0, ZKHIP_ERR_DEVICE, "no HIP device available (libzkhip has no CPU fallback)");
        require(device >= 0 && device < n, ZKHIP_ERR_BAD_ARG, "device index out of range");
        dev_set(device);
        lap("set device");
        std::unique_ptr<zkhip_ctx> ctx(new zkhip_ctx());
        ctx->device = device;
        ctx->stream = stream_create_high_priority();
        lap("first stream");

        ctx->ws = ctx->stream;
        ctx->serial = getenv("ZKHIP_SERIAL") != nullptr;
        ctx->msm.msm_c_env = env_int("ZKHIP_MSM_C", 2, MSM_MAX_C, 0);
        ctx->msm.msm_sets = env_int("ZKHIP_MSM_SETS", 1, 64, 0);
        ctx->msm.msm_waves = env_int("ZKHIP_MSM_WAVES", 1, 8, 0);
        ctx->ntt_single_max = env_int("ZKHIP_NTT_SINGLE_MAX_LOG", 0, NTT_MAX_SUBLOG, 10);
        ctx->ntt_max_sublog = env_int("ZKHIP_NTT_MAX_SUBLOG", 2, NTT_MAX_SUBLOG, NTT_MAX_SUBLOG);
        ctx->ntt_cols = env_int("ZKHIP_NTT_COLS", 1, 8, 2);
        if (ctx->ntt_cols & (ctx->ntt_cols - 1)) ctx->ntt_cols = 2;   // the cols pass has no tail handling: a power of two only
        ctx->nslots = env_int("ZKHIP_SLOTS", 1, ZK_NSLOTS, 3);
        ctx->z_gate = env_int("ZKHIP_Z_GATE", 0, 2, 1);
        ctx->g2_head_start = env_int("ZKHIP_G2_HEAD_START", 0, 2, 1);
        ctx->split_min_log = env_int("ZKHIP_SPLIT_MIN_LOG", 0, 40, 18);
        ctx->fuse_z = env_int("ZKHIP_FUSE_Z", 0, 1, 1) != 0;
        ctx->msm.heavy_runs = env_int("ZKHIP_MSM_HEAVY_RUNS", 0, 1, 1) != 0;
        { const int hg = env_int("ZKHIP_FOLD_HG", 1, 256, 32); ctx->msm.fold_hg = 1 << ilog2_floor((u64)hg); }
        ctx->msm.msm_fused_waves = env_int("ZKHIP_MSM_FUSED_WAVES", 1, 8, 0);
        ctx->msm.msm_g1_waves = env_int("ZKHIP_MSM_G1_WAVES", 1, 16, 0);
        ctx->msm.msm_g2_waves = env_int("ZKHIP_MSM_G2_WAVES", 1, 16, 0);
        ctx->msm.sort_wgs = (u32)env_int("ZKHIP_SORT_WGS", 16, 4096, 256);
        ctx->ntt_fuse_first = env_int("ZKHIP_NTT_FUSE_FIRST", 0, 1, 1);
        if (const char* e = getenv("ZKHIP_PIPES")) ctx->pipe_plan = (e[0] == '-' || e[0] == '0') ? "" : (e[0] == '1' && !e[1]) ? ZK_PIPE_PLAN_RESIDENT : e;
        // every (slot, lane) has a stream of its own: with one stream per lane shared by the slots, the accumulation of
        // proof i+1 queued behind the latency-bound fold tail of proof i on the same lane (a kernel trace showed a lone
        // fold workgroup holding the machine 16 % of the time).  Slot 0 — the one single proofs and the primitives use — is
        // made now, the others when a batch call first needs them (slot_init: 20 ms of stream and event creation each, which a
        // one-proof process never spends).
        ctx->g2_first = env_int("ZKHIP_G2_PRIORITY", 0, 1, 1) != 0;
        slot_init(ctx.get(), ctx->slots[0]);
        lap("slot 0: events");
#ifdef ZK_EMU
        ctx->desc = "zkhip TEST EMULATOR (not a product build)";
#else
        hipDeviceProp_t prop;
        ZK_HIP_CHECK(hipGetDeviceProperties(&prop, device));
        char buf[256];
        snprintf(buf, sizeof(buf), "zkhip on %s (%s), %d CUs, %.0f GiB", prop.name, prop.gcnArchName, prop.multiProcessorCount,
                 prop.totalGlobalMem / 1073741824.0);
        ctx->desc = buf;
        ctx->msm.cus = std::max(1, prop.multiProcessorCount);
        lap("device properties");
#endif
        *out = ctx.release();
    });
}
void zkhip_ctx_free(zkhip_ctx* ctx) {
    if (!ctx) return;
    try {
        dev_set(ctx->device);   // the calling thread may be bound to another device
    } catch (...) {
    }
    dev_sync_all();
    if (ctx->queue) ctx->queue->ctx = nullptr;      // (a queue left open: its zkhip_queue_close only frees the handle)
    staging_drain();          // (the device's staging ring may still track transfers recorded on this context's streams)
    for (auto& sl : ctx->slots) {
        // (streams first, whether or not the slot was ever used: a stream plan makes the streams of every slot at the first proof)
        for (int k = 0; k < ZK_NLANES; ++k)
            if (sl.lanes[k].made) stream_destroy(sl.lanes[k].stream);
        host_free_pinned(sl.h_inputs);
        if (!sl.ready) continue;
        for (auto& so : sl.sorts) event_destroy(so.ready);
        for (int k = 0; k < ZK_NLANES; ++k) {
            event_destroy(sl.lanes[k].done);
            event_destroy(sl.acc_b[k]);
            event_destroy(sl.acc_e[k]);
        }
        for (auto& e : sl.ev) event_destroy(e);
        event_destroy(sl.ntt_b);
        event_destroy(sl.ntt_e);
        event_destroy(sl.g1_go);
        host_free_pinned(sl.h_ws);
    }
    for (Event e : ctx->shard.packed) if (e) event_destroy(e);
    for (Stream q : ctx->idle_streams) stream_destroy(q);
    if (ctx->ntt_lone_made) stream_destroy(ctx->ntt_lone_stream);
    if (ctx->out_made) stream_destroy(ctx->out_stream);
    if (ctx->ntt_made) stream_destroy(ctx->ntt_stream);
    if (ctx->verify_made) stream_destroy(ctx->verify_stream);
    if (ctx->exec_made) stream_destroy(ctx->exec_stream);
    stream_destroy(ctx->stream);
    delete ctx;
}
int32_t zkhip_ctx_clock_probe(zkhip_ctx* ctx, uint32_t duration_us, double* ghz_out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(ghz_out && duration_us >= 1 && duration_us <= 10000000, ZKHIP_ERR_BAD_ARG, "null output or duration out of range (1 us .. 10 s)");
        *ghz_out = 0.0;
#ifndef ZK_EMU
        int khz = 0;
        ZK_HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
        require(khz > 0, ZKHIP_ERR_DEVICE, "the device reports no wall-clock rate");
        unsigned long long* h = (unsigned long long*)host_alloc_pinned(16);
        h[0] = h[1] = 0;
        DBuf d;
        d.ensure(16);
        Stream s = stream_create_high_priority();      // (a stream of its own: it runs beside the context's proofs, not behind them)
        hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, (unsigned long long)duration_us * (unsigned long long)khz / 1000ull, (unsigned long long*)d.p);
        ZK_HIP_CHECK(hipMemcpyAsync(h, d.p, 16, hipMemcpyDeviceToHost, s));
        stream_sync(s);
        stream_destroy(s);
        if (h[1]) *ghz_out = (double)h[0] / ((double)h[1] / ((double)khz * 1e3)) / 1e9;
        host_free_pinned(h);
#endif
    });
}
int32_t zkhip_ctx_tune(zkhip_ctx* ctx, int32_t which, int32_t value) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        auto in = [&](int lo, int hi) { require(value >= lo && value <= hi, ZKHIP_ERR_BAD_ARG, "tunable value out of range"); };
        switch (which) {
            case ZKHIP_TUNE_MSM_C: if (value) in(2, MSM_MAX_C); ctx->msm.msm_c_env = value; break;
            case ZKHIP_TUNE_MSM_SETS: in(0, 64); ctx->msm.msm_sets = value; break;
            case ZKHIP_TUNE_SKIP_INF: in(0, 2); ctx->msm.skip_inf_mode = value; break;
            case ZKHIP_TUNE_B_SORT: in(0, 2); ctx->b_sort_mode = value; break;
            case ZKHIP_TUNE_HEAVY_RUNS: in(0, 1); ctx->msm.heavy_runs = value != 0; break;
            case ZKHIP_TUNE_MSM_WAVES: in(0, 8); ctx->msm.msm_waves = value; break;
            case ZKHIP_TUNE_MSM_LANES: in(0, 1 << 24); ctx->msm.msm_lanes = (u32)value; break;
            case ZKHIP_TUNE_MSM_MIN_SLICE: in(1, 1 << 20); ctx->msm.msm_min_slice = (u32)value; break;
            case ZKHIP_TUNE_FOLD_SCAN: in(0, 1); ctx->msm.fold_scan = value != 0; break;
            case ZKHIP_TUNE_SERIAL: in(0, 1); dev_sync_all(); ctx->serial = value != 0; break;
            case ZKHIP_TUNE_NTT_SINGLE_MAX_LOG: in(0, NTT_MAX_SUBLOG); dev_sync_all(); ctx->ntt_single_max = value; ctx->plans.clear(); break;
            case ZKHIP_TUNE_NTT_MAX_SUBLOG: in(2, NTT_MAX_SUBLOG); dev_sync_all(); ctx->ntt_max_sublog = value; ctx->plans.clear(); break;
            case ZKHIP_TUNE_SLOTS: in(1, ZK_NSLOTS); dev_sync_all(); ctx->nslots = value; break;
            case ZKHIP_TUNE_Z_GATE: in(0, 2); ctx->z_gate = value; break;
            case ZKHIP_TUNE_NTT_FUSE_FIRST: in(0, 1); ctx->ntt_fuse_first = value; break;
            case ZKHIP_TUNE_PIPE_PLAN:
                in(0, 1);
                require(!ctx->pipes_made, ZKHIP_ERR_BAD_ARG, "the streams of this context exist already: the plan is chosen before its first proof");
                if (!getenv("ZKHIP_PIPES")) ctx->pipe_plan = value ? ZK_PIPE_PLAN_RESIDENT : "";
                break;
            case ZKHIP_TUNE_FOLD_HG: in(1, 256); ctx->msm.fold_hg = 1 << ilog2_floor((u64)value); break;
            case ZKHIP_TUNE_FUSE_Z: in(0, 1); ctx->fuse_z = value != 0; break;
            case ZKHIP_TUNE_MSM_FUSED_WAVES: in(0, 8); ctx->msm.msm_fused_waves = value; break;
            case ZKHIP_TUNE_STREAM_JITTER: in(0, 5000); dev_sync_all(); jitter_state().max_us.store(value); break;
            case ZKHIP_TUNE_NTT_COLS:
                in(1, 8);
                require((value & (value - 1)) == 0, ZKHIP_ERR_BAD_ARG, "NTT_COLS must be 1, 2, 4 or 8 (the cols pass covers N2 / cols workgroups exactly)");
                dev_sync_all(); ctx->ntt_cols = value; ctx->plans.clear(); break;
            case ZKHIP_TUNE_EXEC_CHUNK: in(0, 65535 * (int)WX_BLOCK); ctx->exec_chunk = value; break;      // (the gathers' grids hold the waves of a chunk along y)
            case ZKHIP_TUNE_EXEC_WIDE: in(0, 1); ctx->exec_wide = value != 0; break;      // (read at each zkhip_compute_witness; changes no result)
            case ZKHIP_TUNE_EXEC_WIDE_MIN: in(0, EXEC_WIDE_MIN_MAX); ctx->exec_wide_min = value; break;
            case ZKHIP_TUNE_ALLOC_FILL: dev_sync_all(); alloc_fill_word().store((uint32_t)value); break;   // (tests only, process-wide: devrt.h)
            default: throw ApiError{ZKHIP_ERR_BAD_ARG, "unknown tunable"};
        }
    });
}
const char* zkhip_last_error(const zkhip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int32_t zkhip_describe(const zkhip_ctx* ctx, char* buf, size_t cap) {
    if (!ctx || !buf || !cap) return ZKHIP_ERR_BAD_ARG;
    snprintf(buf, cap, "%s", ctx->desc.c_str());
    return ZKHIP_OK;
}

int32_t zkhip_pk_load_g16(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_pk** out) { return load_key(ctx, curve, 0, bytes, len, 0, 1, out); }
int32_t zkhip_pk_load_g16_shard(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, uint32_t rank, uint32_t world, zkhip_pk** out) {
    return load_key(ctx, curve, 0, bytes, len, rank, world, out);
}
int32_t zkhip_pk_load_gm17(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_pk** out) { return load_key(ctx, curve, 1, bytes, len, 0, 1, out); }
int32_t zkhip_pk_load_gm17_shard(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, uint32_t rank, uint32_t world, zkhip_pk** out) {
    return load_key(ctx, curve, 1, bytes, len, rank, world, out);
}
void zkhip_pk_free(zkhip_pk* pk) { delete pk; }
int32_t zkhip_pk_bind_r1cs(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* r1cs) {
    return bind_key(ctx, pk, r1cs, true, [&](const CurveOps* ops, bool& started) {
        started = true;
        ops->pk_bind(ctx, pk, r1cs);
    });
}
int32_t zkhip_pk_unbind(zkhip_pk* pk) {
    if (!pk) return ZKHIP_ERR_BAD_ARG;
    return guarded(pk->ctx, [&] { ops_for(pk->curve)->pk_unbind(pk); });
}
// a shard of a multi-GPU key (or a whole key): the binding computed from the key FILE — the transforms need every base once — of
// which this key keeps its own index ranges
int32_t zkhip_pk_bind_r1cs_shard(zkhip_ctx* ctx, zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* key_bytes, size_t len) {
    return bind_key(ctx, pk, r1cs, key_bytes != nullptr, [&](const CurveOps* ops, bool& started) {
        std::vector<uint8_t> h_host, l_host;
        u64 fp[2];
        ops->bound_level0_from_file(ctx, pk->scheme, r1cs, key_bytes, len, h_host, l_host, fp);
        started = true;
        ops->install_bound_ranges(ctx, pk, r1cs, h_host.data(), h_host.size(), l_host.data(), l_host.size(), fp);
    });
}
// One rank's share of a proof whose witness map is split between the ranks of a multi-PROCESS prover (one process per GPU): begin
// computes this rank's half — `half` = 0: a, 1: b on the coset, N x 32 bytes (R'-form, packed) into `half_out` (host memory) — and
// leaves the proof in flight; the ranks exchange halves (partners of the other parity); end takes the partner's and finishes.
int32_t zkhip_prove_g16_split_begin(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident, const uint8_t* r,
                                    const uint8_t* s, int32_t half, uint8_t* half_out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && (z || z_resident) && r && s && half_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        if (!z) require(z_resident->ctx == ctx && z_resident->curve == pk->curve && z_resident->m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG,
                        "assignment does not match the constraint system");
        for (auto& sl : ctx->slots) require(!sl.busy, ZKHIP_ERR_BAD_ARG, "a proof is in flight in this context");
        const CurveOps* ops = ops_for(pk->curve);
        try {
            ops->split_begin(ctx, pk, r1cs, z, z ? nullptr : z_resident->scalars.p, r, s, half);
            ops->split_half_out(ctx, pk, half_out);
        } catch (...) {
            split_drop(ctx);      // (a begin that fails leaves nothing pending)
            throw;
        }
    });
}
int32_t zkhip_prove_g16_split_end(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* other_half, uint8_t* partial_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && other_half && partial_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        // the state and the handles first, on the host: a call that is refused for them leaves the pending proof as it is
        const ProofSlot& sl = ctx->slots[0];
        require(sl.split_pending, ZKHIP_ERR_BAD_ARG, "no split proof pending in this context: zkhip_prove_g16_split_begin comes first, and a proof is collected once");
        require(sl.split_pk == pk && sl.split_cs == r1cs, ZKHIP_ERR_BAD_ARG,
                "the split proof pending in this context was begun with another proving key or constraint system");
        const CurveOps* ops = ops_for(pk->curve);
        try {
            ops->split_fetch_host(ctx, pk, other_half);
            ops->split_end_partial(ctx, pk, r1cs, partial_out, timings);
        } catch (...) {
            split_drop(ctx);      // (an end that fails leaves nothing pending either)
            throw;
        }
    }, true);
}
int32_t zkhip_prove_g16_split_abort(zkhip_ctx* ctx) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] { split_drop(ctx); }, true);
}
int32_t zkhip_r1cs_fingerprint(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, uint64_t out[2]) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        u64 fp[2];
        ops_for(r1cs->curve)->r1cs_fingerprint(ctx, r1cs, fp);
        out[0] = fp[0]; out[1] = fp[1];
    });
}
int32_t zkhip_r1cs_matvec_shape(const zkhip_r1cs* r1cs, int32_t lanes[3], uint64_t* n_long, uint64_t* n_huge) {
    if (!r1cs || !lanes || !n_long || !n_huge) return ZKHIP_ERR_BAD_ARG;
    int g[3];
    matvec_lanes(r1cs, g);
    for (int k = 0; k < 3; ++k) lanes[k] = g[k];
    *n_long = r1cs->n_long - r1cs->n_huge;      // (the list of long rows begins with the huge ones)
    *n_huge = r1cs->n_huge;
    return ZKHIP_OK;
}
int32_t zkhip_pk_is_bound(const zkhip_pk* pk, const zkhip_r1cs* r1cs) {
    if (!pk || !r1cs) return 0;
    return pk->bound_uid != 0 && pk->bound_uid == r1cs->uid ? 1 : 0;
}
int32_t zkhip_pk_dims(const zkhip_pk* pk, uint64_t out[4]) {
    if (!pk || !out) return ZKHIP_ERR_BAD_ARG;
    out[0] = pk->m; out[1] = pk->hlen; out[2] = pk->w; out[3] = pk->l;
    return ZKHIP_OK;
}

int32_t zkhip_r1cs_load(zkhip_ctx* ctx, int32_t curve, uint64_t n, uint64_t l, uint64_t w, const uint64_t* rowptr_a, const uint32_t* col_a,
                        const uint8_t* val_a, const uint64_t* rowptr_b, const uint32_t* col_b, const uint8_t* val_b, const uint64_t* rowptr_c,
                        const uint32_t* col_c, const uint8_t* val_c, zkhip_r1cs** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(out && rowptr_a && rowptr_b && rowptr_c, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(l >= 1, ZKHIP_ERR_BAD_ARG, "num_instance must be >= 1 (the constant ONE)");
        require(l + w + 2 < ((u64)1 << 31) && n < ((u64)1 << 31), ZKHIP_ERR_BAD_ARG, "constraint system too large");
        std::unique_ptr<zkhip_r1cs> cs(new zkhip_r1cs());
        cs->curve = curve; cs->ctx = ctx; cs->n = n; cs->l = l; cs->w = w;
        cs->logN = ilog2_ceil(n + l);
        cs->N = (u64)1 << cs->logN;
        const u64* rp[3] = {rowptr_a, rowptr_b, rowptr_c};
        const u32* col[3] = {col_a, col_b, col_c};
        const uint8_t* val[3] = {val_a, val_b, val_c};
        ops_for(curve)->r1cs_load(ctx, cs.get(), rp, col, val);
        *out = cs.release();
    });
}
void zkhip_r1cs_free(zkhip_r1cs* cs) { delete cs; }

int32_t zkhip_prove_g16(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, const uint8_t* r, const uint8_t* s,
                        uint8_t* proof_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && z && r && s && proof_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_g16_partial + zkhip_combine_g16");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        ops_for(pk->curve)->prove(ctx, pk, r1cs, z, nullptr, r, s, proof_out, timings);
    });
}

int32_t zkhip_assignment_upload(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && z && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        std::unique_ptr<zkhip_assignment> a(new zkhip_assignment());
        a->curve = r1cs->curve; a->ctx = ctx; a->m = r1cs->l + r1cs->w;
        ops_for(r1cs->curve)->assignment_upload(ctx, a.get(), z);
        *out = a.release();
    });
}
void zkhip_assignment_free(zkhip_assignment* a) { delete a; }

// ---- compact assignments: the host-only packer / unpacker (no context), and the upload from the packed form
// (the kernel clamps nothing: what the host validates per block must be what one workgroup takes)
static_assert(ZPACK_BLOCK == ZPACK_BLOCK_ELEMS, "the host validates blocks of the size the kernel widens");
int32_t zkhip_assignment_pack_bound(uint64_t m, uint64_t* bytes) {
    if (!bytes || m >= (uint64_t)1 << 56) { g_create_err = "bad argument"; return ZKHIP_ERR_BAD_ARG; }
    *bytes = packed_layout(m, 32 * m).total;      // every element 32 bytes wide: no block needs padding
    return ZKHIP_OK;
}
int32_t zkhip_assignment_pack(const uint8_t* z, uint64_t m, uint8_t* out, uint64_t cap, uint64_t* len) {
    if ((!z && m) || !out || !len) { g_create_err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    return guarded_host([&] { assignment_pack(z, m, out, cap, len); });
}
int32_t zkhip_assignment_unpack(const uint8_t* packed, size_t len, uint8_t* z_out, uint64_t m_cap, uint64_t* m) {
    if (!packed || !m) { g_create_err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    return guarded_host([&] {
        const PackedLayout ly = assignment_packed_validate(packed, len);
        *m = ly.m;
        if (ly.m > m_cap || (!z_out && ly.m)) throw IngestError{ZKHIP_ERR_BAD_ARG, "z_out holds " + std::to_string(m_cap) + " elements, the packed assignment has " + std::to_string(ly.m)};
        assignment_unpack(packed, ly, z_out);
    });
}
int32_t zkhip_prog_assignment_packed(const zkhip_prog* prog, const uint8_t* witness, size_t len, uint8_t* packed_out, uint64_t cap,
                                     uint64_t* packed_len, uint8_t* inputs_out, uint64_t inputs_cap, uint64_t* n_inputs) {
    if (!prog || !witness || !packed_out || !packed_len) { g_create_err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    return guarded_host([&] { prog_assignment_packed(prog, witness, len, packed_out, cap, packed_len, inputs_out, inputs_cap, n_inputs); });
}
int32_t zkhip_assignment_upload_packed(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* packed, size_t len, zkhip_assignment** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && packed && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        // the whole structure on the host, before anything is enqueued: the kernel never sees an inconsistent buffer
        PackedLayout ly;
        try {
            ly = assignment_packed_validate(packed, len);
        } catch (const IngestError& e) {
            throw ApiError{e.code, e.msg};
        }
        const std::string dims = "the packed assignment has " + std::to_string(ly.m) + " elements, the constraint system " + std::to_string(r1cs->l + r1cs->w) + " variables (l + w)";
        require(ly.m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG, dims.c_str());
        require(packed_first_is_one(packed, ly), ZKHIP_ERR_BAD_ARG, Z0_NOT_ONE_MSG);
        std::unique_ptr<zkhip_assignment> a(new zkhip_assignment());
        a->curve = r1cs->curve; a->ctx = ctx; a->m = ly.m;
        ops_for(r1cs->curve)->assignment_upload_packed(ctx, a.get(), packed, len, ly.tags_off, ly.index_off, ly.payload_off);
        *out = a.release();
    });
}

// ---- witness files on the device: the plan (two id -> column tables, resident), and the upload through it
int32_t zkhip_wplan_create(zkhip_ctx* ctx, const zkhip_prog* prog, const zkhip_r1cs* r1cs, zkhip_wplan** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {      // (the gate: it enqueues copies, so it is refused while a split proof or a queue is pending)
        require(prog && r1cs && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        std::shared_ptr<WPlanTables> host(new WPlanTables());
        try {
            wplan_build(*prog, r1cs->curve, r1cs->l, r1cs->w, *host);
        } catch (const IngestError& e) {
            throw ApiError{e.code, e.msg};
        }
        std::unique_ptr<zkhip_wplan> plan(new zkhip_wplan());
        plan->ctx = ctx;
        plan->cs_uid = r1cs->uid;
        plan->pos.ensure(std::max<size_t>(host->pos.size(), 1) * 4);
        plan->neg.ensure(std::max<size_t>(host->neg.size(), 1) * 4);
        dev_h2d(plan->pos.p, host->pos.data(), host->pos.size() * 4, ctx->stream);
        if (!host->neg.empty()) dev_h2d(plan->neg.p, host->neg.data(), host->neg.size() * 4, ctx->stream);
        stream_sync(ctx->stream);
        plan->host = host;
        *out = plan.release();
    });
}
void zkhip_wplan_free(zkhip_wplan* plan) { delete plan; }
// the public inputs out of the head of z (l x 32 B), in the order of public_inputs_values
static void witness_inputs(const WPlanTables& t, const uint8_t* head, uint8_t* inputs_out) {
    for (size_t k = 0; k < t.input_cols.size(); ++k) memcpy(inputs_out + 32 * k, head + 32 * (size_t)t.input_cols[k], 32);
}
int32_t zkhip_assignment_upload_witness(zkhip_ctx* ctx, const zkhip_wplan* plan, const uint8_t* witness, size_t len, uint8_t* inputs_out, uint64_t inputs_cap,
                                        uint64_t* n_inputs, zkhip_assignment** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(out != nullptr, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        if (n_inputs) *n_inputs = 0;
        const WitnessZ wz = witness_source(ctx, plan, nullptr, witness, len);
        const WPlanTables& t = *plan->host;
        require(!inputs_out || inputs_cap >= t.input_cols.size(), ZKHIP_ERR_BAD_ARG, "inputs buffer too small");
        std::unique_ptr<zkhip_assignment> a(new zkhip_assignment());
        a->curve = t.curve; a->ctx = ctx; a->m = t.l + t.w;
        std::vector<uint8_t> head(inputs_out ? t.l * 32 : 0);
        ops_for(t.curve)->assignment_upload_witness(ctx, a.get(), wz, inputs_out ? head.data() : nullptr);
        if (inputs_out) witness_inputs(t, head.data(), inputs_out);
        if (n_inputs) *n_inputs = t.input_cols.size();
        *out = a.release();
    });
}

// ---- witnesses computed on the device: the plan (the program's statements compiled for k_exec_program, resident), and the call
static bool scalar_canonical(int curve, const uint8_t* b) {
    if (curve == ZKHIP_CURVE_BN128) return canon_lt_mod(fe_from_bytes_canon<Fe<Bn254Fr>>(b));
    if (curve == ZKHIP_CURVE_BLS12_381) return canon_lt_mod(fe_from_bytes_canon<Fe<Bls381Fr>>(b));
    return canon_lt_mod(fe_from_bytes_canon<Fe<Bls377Fr>>(b));
}
int32_t zkhip_xplan_create(zkhip_ctx* ctx, const zkhip_prog* prog, const zkhip_r1cs* r1cs, const uint8_t* out_bytes, size_t len, zkhip_xplan** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {      // (the gate: it enqueues the copies of its tables, as zkhip_wplan_create does)
        require(prog && r1cs && out_bytes && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        std::shared_ptr<XPlanHost> host(new XPlanHost());
        try {
            xplan_build(*prog, r1cs->curve, r1cs->l, r1cs->w, r1cs->n, out_bytes, len, *host);
        } catch (const IngestError& e) {
            throw ApiError{e.code, e.msg};
        }
        std::unique_ptr<zkhip_xplan> plan(new zkhip_xplan());
        plan->ctx = ctx;
        auto up = [&](DBuf& d, const void* src, size_t bytes) {
            d.ensure(std::max<size_t>(bytes, 16));
            if (bytes) dev_h2d(d.p, src, bytes, ctx->stream);
        };
        up(plan->code, host->code.data(), host->code.size() * 4);
        up(plan->pool, host->pool.data(), host->pool.size() * 4);
        up(plan->file_ids, host->file_ids.data(), host->file_ids.size() * 8);
        up(plan->file_slots, host->file_slots.data(), host->file_slots.size() * 4);
        up(plan->input_cols, host->input_cols.data(), host->input_cols.size() * 4);
        up(plan->sched, host->sched.data(), host->sched.size() * 4);
        up(plan->level_start, host->level_start.data(), host->level_start.size() * 4);
        stream_sync(ctx->stream);
        plan->host = host;
        *out = plan.release();
    });
}
void zkhip_xplan_free(zkhip_xplan* plan) { delete plan; }
int32_t zkhip_xplan_dims(const zkhip_xplan* plan, uint64_t out[8]) {
    if (!plan || !out) return ZKHIP_ERR_BAD_ARG;
    plan->host->dims(out);
    return ZKHIP_OK;
}
int32_t zkhip_xplan_levels(const zkhip_xplan* plan, uint64_t out[4]) {
    if (!plan || !out) return ZKHIP_ERR_BAD_ARG;
    plan->host->levels(out);
    return ZKHIP_OK;
}
int32_t zkhip_exec_last(const zkhip_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return ZKHIP_ERR_BAD_ARG;
    for (int k = 0; k < 4; ++k) out[k] = ctx->exec_last[k];
    return ZKHIP_OK;
}
// (on its own stream and in its own buffers, as the pairing checks: allowed while a proof queue is open, refused while a split proof
// is pending — guarded_verify is that gate)
int32_t zkhip_compute_witness(zkhip_ctx* ctx, const zkhip_xplan* plan, uint32_t count, const uint8_t* args, zkhip_assignment** assignments_out,
                              uint8_t* witness_out, uint64_t witness_cap_each, uint8_t* inputs_out, uint64_t inputs_cap_each, int32_t* status,
                              uint64_t* first_statement, uint64_t* first_row) {
    bool unsatisfied = false;
    const int32_t rc = guarded_verify(ctx, [&] {
        require(plan != nullptr, ZKHIP_ERR_BAD_ARG, "null argument");
        require(plan->ctx == ctx, ZKHIP_ERR_BAD_ARG, "the execution plan belongs to another context");
        if (count == 0) return;
        const XPlanHost& h = *plan->host;
        require(status && (args || h.n_args == 0), ZKHIP_ERR_BAD_ARG, "null argument");
        require(!witness_out || witness_cap_each >= h.file_bytes(), ZKHIP_ERR_BAD_ARG,
                ("witness buffer too small: a file of this program has " + std::to_string(h.file_bytes()) + " bytes (8 + 40 x zkhip_xplan_dims [5])").c_str());
        require(!inputs_out || inputs_cap_each >= h.input_cols.size(), ZKHIP_ERR_BAD_ARG, "inputs buffer too small");
        // every argument below r, before anything is enqueued
        const CurveOps* ops = ops_for(h.curve);
        for (uint64_t i = 0; i < count; ++i)
            for (uint64_t k = 0; k < h.n_args; ++k)
                if (!scalar_canonical(h.curve, args + (i * h.n_args + k) * 32))
                    throw ApiError{ZKHIP_ERR_PARSE, "instance " + std::to_string(i) + ", argument " + std::to_string(k) + ": not a canonical field element (at or above r)"};
        std::vector<std::unique_ptr<zkhip_assignment>> made(assignments_out ? count : 0);
        if (assignments_out) for (uint32_t i = 0; i < count; ++i) assignments_out[i] = nullptr;
        std::vector<uint64_t> own_st(first_statement ? 0 : count), own_row(first_row ? 0 : count);      // (the message names both, asked for or not)
        if (!first_statement) first_statement = own_st.data();
        if (!first_row) first_row = own_row.data();
        const uint64_t bad = ops->compute_witness(ctx, plan, count, args, assignments_out ? &made : nullptr, witness_out, witness_cap_each, inputs_out, inputs_cap_each,
                                                  status, first_statement, first_row);
        if (assignments_out) for (uint32_t i = 0; i < count; ++i) assignments_out[i] = made[i].release();
        if (bad) {
            uint32_t i = 0;
            while (status[i] == ZKHIP_OK) ++i;
            ctx->err = "instance " + std::to_string(i) + " does not satisfy the program: statement " + std::to_string(first_statement[i]) + ", constraint (R1CS row) " +
                       std::to_string(first_row[i]) + "; " + std::to_string(bad) + " of " + std::to_string(count) + " instances failed";
            unsatisfied = true;
        }
    });
    return rc == ZKHIP_OK && unsatisfied ? ZKHIP_ERR_UNSATISFIED : rc;
}

int32_t zkhip_prove_g16_resident(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_assignment* z, const uint8_t* r,
                                 const uint8_t* s, uint8_t* proof_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && z && r && s && proof_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_g16_partial + zkhip_combine_g16");
        require(pk->ctx == ctx && r1cs->ctx == ctx && z->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        require(z->curve == pk->curve && z->m == pk->m, ZKHIP_ERR_BAD_ARG, "assignment does not match the proving key");
        ops_for(pk->curve)->prove(ctx, pk, r1cs, nullptr, z->scalars.p, r, s, proof_out, timings);
    });
}

int32_t zkhip_partial_size(int32_t curve, uint64_t* bytes) {
    if (!bytes) return ZKHIP_ERR_BAD_ARG;
    try {
        *bytes = ops_for(curve)->partial_bytes;
    } catch (...) {
        return ZKHIP_ERR_BAD_ARG;
    }
    return ZKHIP_OK;
}
int32_t zkhip_prove_g16_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident,
                                const uint8_t* r, const uint8_t* s, uint8_t* partial_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && (z || z_resident) && r && s && partial_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        if (!z) require(z_resident->ctx == ctx && z_resident->curve == pk->curve && z_resident->m == pk->m, ZKHIP_ERR_BAD_ARG,
                        "assignment does not match the proving key");
        ops_for(pk->curve)->prove_partial(ctx, pk, r1cs, z, z ? nullptr : z_resident->scalars.p, r, s, partial_out, timings);
    });
}
int32_t zkhip_combine_g16(zkhip_ctx* ctx, const zkhip_pk* pk, uint32_t count, const uint8_t* partials, const uint8_t* r, const uint8_t* s,
                          uint8_t* proof_out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && partials && r && s && proof_out && count >= 1, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->scheme == 0, ZKHIP_ERR_BAD_ARG, "this is a GM17 proving key");
        ops_for(pk->curve)->combine(pk, count, partials, r, s, proof_out);
    }, true);      // (host arithmetic only: legal beside a pending split proof)
}

int32_t zkhip_prove_g16_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count, const uint8_t* z, const uint8_t* rs,
                              uint8_t* proofs_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && rs && proofs_out && (z || count == 0), ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_g16_partial + zkhip_combine_g16");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        ops_for(pk->curve)->prove_batch(ctx, pk, r1cs, count, z, nullptr, rs, proofs_out, timings);
    });
}
int32_t zkhip_prove_g16_resident_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count, zkhip_assignment* const* zs,
                                       const uint8_t* rs, uint8_t* proofs_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && rs && proofs_out && (zs || count == 0), ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: use zkhip_prove_g16_partial + zkhip_combine_g16");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        std::vector<void*> dev(count);
        for (uint32_t i = 0; i < count; ++i) {
            require(zs[i] && zs[i]->ctx == ctx && zs[i]->curve == pk->curve && zs[i]->m == pk->m, ZKHIP_ERR_BAD_ARG,
                    "assignment does not match the proving key");
            dev[i] = zs[i]->scalars.p;
        }
        ops_for(pk->curve)->prove_batch(ctx, pk, r1cs, count, nullptr, dev.data(), rs, proofs_out, timings);
    });
}

// ---- checked proving
int32_t zkhip_r1cs_check(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident, uint64_t* first_row, uint64_t* n_bad) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && (z || z_resident), ZKHIP_ERR_BAD_ARG, "null argument");
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        if (!z) require(z_resident->ctx == ctx && z_resident->curve == r1cs->curve && z_resident->m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG,
                        "assignment does not match the constraint system");
        u64 v[2] = {~(u64)0, 0};
        ops_for(r1cs->curve)->r1cs_check(ctx, r1cs, z, z ? nullptr : z_resident->scalars.p, v);
        if (first_row) *first_row = v[0];
        if (n_bad) *n_bad = v[1];
        if (v[1]) {
            char msg[160];
            snprintf(msg, sizeof(msg), "constraint %llu of %llu is not satisfied (%llu in all)", (unsigned long long)v[0], (unsigned long long)r1cs->n,
                     (unsigned long long)v[1]);
            throw ApiError{ZKHIP_ERR_UNSATISFIED, msg};
        }
    });
}
int32_t zkhip_ctx_set_checked(zkhip_ctx* ctx, int32_t on) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    const int32_t was = ctx->checked ? 1 : 0;
    if (on >= 0 && split_pending(ctx)) {
        ctx->err = SPLIT_PENDING_MSG;
        return ZKHIP_ERR_BAD_ARG;
    }
    if (on >= 0 && ctx->queue) {      // (an open queue read the mode when it was opened)
        ctx->err = QUEUE_OPEN_MSG;
        return ZKHIP_ERR_BAD_ARG;
    }
    if (on >= 0) ctx->checked = on != 0;
    return was;
}
int32_t zkhip_ctx_unsatisfied(const zkhip_ctx* ctx, uint32_t cap, uint32_t* proof_idx, uint64_t* first_row, uint64_t* n_bad, uint32_t* count) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    for (size_t k = 0; k < ctx->unsat.size() && k < cap; ++k) {
        if (proof_idx) proof_idx[k] = ctx->unsat[k].proof;
        if (first_row) first_row[k] = ctx->unsat[k].first_row;
        if (n_bad) n_bad[k] = ctx->unsat[k].n_bad;
    }
    if (count) *count = (uint32_t)ctx->unsat.size();
    return ZKHIP_OK;
}

// ---- the proof queue: ctx->nslots proofs in flight ACROSS calls (the helpers above hold the rules)
int32_t zkhip_queue_open(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_queue** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {      // (the gate: refused while a split proof is pending or another queue is open)
        require(pk && r1cs && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        require(pk->world == 1, ZKHIP_ERR_BAD_ARG, "this proving key is one shard of a multi-GPU key: a proof queue takes a whole key");
        for (auto& sl : ctx->slots) require(!sl.busy, ZKHIP_ERR_BAD_ARG, "a proof is in flight in this context");
        ops_for(pk->curve)->queue_check(pk, r1cs);
        std::unique_ptr<zkhip_queue> q(new zkhip_queue());
        q->ctx = ctx;
        q->pk = pk;
        q->cs = r1cs;
        q->cap = (u32)std::max(1, std::min(ctx->nslots, ZK_NSLOTS));
        q->checked = ctx->checked;
        ctx->queue = q.get();
        *out = q.release();
    });
}
int32_t zkhip_queue_state(const zkhip_queue* q, uint32_t* capacity, uint32_t* in_flight) {
    if (!q) return ZKHIP_ERR_BAD_ARG;
    if (capacity) *capacity = q->cap;
    if (in_flight) *in_flight = (uint32_t)(q->next - q->head);
    return ZKHIP_OK;
}
int32_t zkhip_queue_submit(zkhip_queue* q, const uint8_t* z, zkhip_assignment* z_resident, const uint8_t* rnd, uint64_t* ticket) {
    return queue_submit(q, z, z_resident, nullptr, 0, false, rnd, ticket);
}
int32_t zkhip_queue_submit_packed(zkhip_queue* q, const uint8_t* packed, size_t len, const uint8_t* rnd, uint64_t* ticket) {
    return queue_submit(q, nullptr, nullptr, packed, len, true, rnd, ticket);
}
int32_t zkhip_queue_submit_witness(zkhip_queue* q, const zkhip_wplan* plan, const uint8_t* witness, size_t len, const uint8_t* rnd, uint64_t* ticket) {
    return queue_submit(q, nullptr, nullptr, witness, len, false, rnd, ticket, plan, true);
}
int32_t zkhip_queue_ready(zkhip_queue* q, int32_t* ready) {
    if (!q || !q->ctx || !ready) return ZKHIP_ERR_BAD_ARG;
    *ready = 0;
    if (q->head == q->next) return ZKHIP_OK;                    // nothing to collect
    if (q->broken) { *ready = 1; return ZKHIP_OK; }             // (collect answers at once)
    return queue_guarded(q, [&] { *ready = event_done(q->ctx->slots[q->head % q->cap].ev[3]) ? 1 : 0; });
}
// collect, with or without the public inputs of a ticket that was submitted as a witness file (the head of z in the slot's pinned
// buffer, copied on the stream that wrote it before the slot's first event; permuted here by the plan's host tables)
static int32_t queue_collect(zkhip_queue* q, uint64_t* ticket, uint8_t* proof_out, uint8_t* inputs_out, uint64_t inputs_cap, uint64_t* n_inputs, zkhip_timings* timings) {
    if (!q || !q->ctx) return ZKHIP_ERR_BAD_ARG;
    zkhip_ctx* ctx = q->ctx;
    if (n_inputs) *n_inputs = 0;
    if (!proof_out) { ctx->err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    if (q->head == q->next) { ctx->err = "the proof queue is empty: nothing to collect"; return ZKHIP_ERR_BAD_ARG; }
    if (!q->broken && inputs_out) {      // (before the ticket is spent: a refusal for the caller's buffer changes nothing)
        const ProofSlot& sl = ctx->slots[q->head % q->cap];
        if (sl.wit && inputs_cap < sl.wit->input_cols.size()) { ctx->err = "inputs buffer too small"; return ZKHIP_ERR_BAD_ARG; }
    }
    const u64 t = q->head++;      // whatever happens to this proof, its ticket is spent
    if (ticket) *ticket = t;
    if (q->broken) { ctx->err = q->dev_err; return ZKHIP_ERR_DEVICE; }
    return queue_guarded(q, [&] {
        ctx->unsat.clear();
        ops_for(q->pk->curve)->queue_finish(ctx, ctx->slots[t % q->cap], q->pk, proof_out, timings);
        if (!ctx->unsat.empty()) {      // (checked mode: `finish` has zero-filled the slot and noted the one triple, proof index 0)
            const auto& u = ctx->unsat.front();
            char msg[200];
            snprintf(msg, sizeof(msg), "ticket %llu: constraint %llu of %llu is not satisfied (%llu in all)", (unsigned long long)t,
                     (unsigned long long)u.first_row, (unsigned long long)q->cs->n, (unsigned long long)u.n_bad);
            throw ApiError{ZKHIP_ERR_UNSATISFIED, msg};
        }
        const ProofSlot& sl = ctx->slots[t % q->cap];
        if (sl.wit) {
            if (inputs_out) witness_inputs(*sl.wit, (const uint8_t*)sl.h_inputs, inputs_out);
            if (n_inputs) *n_inputs = sl.wit->input_cols.size();
        }
    });
}
int32_t zkhip_queue_collect(zkhip_queue* q, uint64_t* ticket, uint8_t* proof_out, zkhip_timings* timings) {
    return queue_collect(q, ticket, proof_out, nullptr, 0, nullptr, timings);
}
int32_t zkhip_queue_collect_inputs(zkhip_queue* q, uint64_t* ticket, uint8_t* proof_out, uint8_t* inputs_out, uint64_t inputs_cap, uint64_t* n_inputs,
                                   zkhip_timings* timings) {
    return queue_collect(q, ticket, proof_out, inputs_out, inputs_cap, n_inputs, timings);
}
int32_t zkhip_queue_close(zkhip_queue* q) {
    if (!q) return ZKHIP_ERR_BAD_ARG;
    if (zkhip_ctx* ctx = q->ctx) {
        if (q->head != q->next && !q->broken) {      // what is uncollected drains and is dropped
            try { dev_set(ctx->device); } catch (...) {}
            dev_sync_all();
            for (auto& sl : ctx->slots) sl.busy = false;
        }
        ctx->queue = nullptr;
    }
    delete q;
    return ZKHIP_OK;
}

int32_t zkhip_ntt(zkhip_ctx* ctx, int32_t curve, uint32_t log_n, int32_t dir, uint8_t* data) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(data && dir >= 0 && dir <= 3, ZKHIP_ERR_BAD_ARG, "bad argument");
        ops_for(curve)->ntt(ctx, log_n, dir, data);
    });
}
int32_t zkhip_witness_map(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* z, uint8_t* h_out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && z && h_out, ZKHIP_ERR_BAD_ARG, "null argument");
        ops_for(r1cs->curve)->witness_map(ctx, r1cs, z, h_out);
    });
}
int32_t zkhip_msm_g1(zkhip_ctx* ctx, int32_t curve, uint64_t n, const uint8_t* bases, const uint8_t* scalars, uint8_t* out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(out && (n == 0 || (bases && scalars)), ZKHIP_ERR_BAD_ARG, "null argument");
        ops_for(curve)->msm_g1(ctx, n, bases, scalars, out);
    });
}
int32_t zkhip_msm_g2(zkhip_ctx* ctx, int32_t curve, uint64_t n, const uint8_t* bases, const uint8_t* scalars, uint8_t* out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(out && (n == 0 || (bases && scalars)), ZKHIP_ERR_BAD_ARG, "null argument");
        ops_for(curve)->msm_g2(ctx, n, bases, scalars, out);
    });
}
int32_t zkhip_field_op(zkhip_ctx* ctx, int32_t curve, int32_t field, int32_t op, uint64_t count, const uint8_t* a, const uint8_t* b,
                       uint8_t* out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(a && b && out && op >= 0 && field >= 0 && field <= 5 && op <= (field < 2 ? 2 : field == 2 ? 4 : field == 3 ? 10 : 15), ZKHIP_ERR_BAD_ARG, "bad argument");
        ops_for(curve)->field_op(ctx, field, op, count, a, b, out);
    });
}
int32_t zkhip_group_op(zkhip_ctx* ctx, int32_t curve, int32_t group, int32_t form, int32_t op, uint64_t count, const uint32_t* a, const uint32_t* b,
                       const uint32_t* k, const uint8_t* flags, uint32_t* out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(a && b && k && flags && out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(group_op_known(group, form, op), ZKHIP_ERR_BAD_ARG, "unknown group, form or operation (or no such operation for this group and form)");
        require(count <= ((u64)1 << 24), ZKHIP_ERR_BAD_ARG, "count too large");
        ops_for(curve)->group_op(ctx, group, form, op, count, a, b, k, flags, out);
    });
}

int32_t zkhip_pairing_products(zkhip_ctx* ctx, int32_t curve, uint64_t count, uint32_t pairs_per_item, const uint8_t* g1, const uint8_t* g2, uint8_t* ok_out) {
    return guarded_verify(ctx, [&] {
        const CurveOps* ops = ops_for(curve);
        if (count == 0) return;
        require(g1 && g2 && ok_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pairs_per_item >= 1 && pairs_per_item <= PAIR_MAX_PAIRS, ZKHIP_ERR_BAD_ARG, "pairs_per_item must be 1 .. 8 (one lane of an item's group per pair)");
        require(count <= ((u64)1 << 24), ZKHIP_ERR_BAD_ARG, "count too large");
        ops->pairing_products(ctx, count, pairs_per_item, g1, g2, ok_out);
    });
}
static int32_t vk_load(zkhip_ctx* ctx, int32_t curve, int scheme, const uint8_t* bytes, size_t len, zkhip_vk** out) {
    return guarded_verify(ctx, [&] {
        require(bytes && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        std::unique_ptr<zkhip_vk> vk(new zkhip_vk());
        vk->curve = curve;
        vk->ctx = ctx;
        ops_for(curve)->vk_load(ctx, scheme, bytes, len, vk.get());
        *out = vk.release();
    });
}
int32_t zkhip_vk_load_g16(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_vk** out) { return vk_load(ctx, curve, 0, bytes, len, out); }
int32_t zkhip_vk_load_gm17(zkhip_ctx* ctx, int32_t curve, const uint8_t* bytes, size_t len, zkhip_vk** out) { return vk_load(ctx, curve, 1, bytes, len, out); }
void zkhip_vk_free(zkhip_vk* vk) { delete vk; }
int32_t zkhip_vk_dims(const zkhip_vk* vk, uint64_t out[2]) {
    if (!vk || !out) return ZKHIP_ERR_BAD_ARG;
    out[0] = vk->nq - 1;
    out[1] = (uint64_t)vk->scheme;
    return ZKHIP_OK;
}
static int32_t verify_batch(zkhip_ctx* ctx, const zkhip_vk* vk, int scheme, uint64_t count, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out) {
    return guarded_verify(ctx, [&] {
        require(vk, ZKHIP_ERR_BAD_ARG, "null argument");
        require(vk->ctx == ctx, ZKHIP_ERR_BAD_ARG, "the verifying key belongs to another context");
        require(vk->scheme == scheme, ZKHIP_ERR_BAD_ARG, scheme ? "a Groth16 verifying key was handed to the GM17 call" : "a GM17 verifying key was handed to the Groth16 call");
        if (count == 0) return;
        require(proofs && ok_out && (inputs || vk->nq == 1), ZKHIP_ERR_BAD_ARG, "null argument");
        require(count <= ((u64)1 << 22) && count * vk->nq <= ((u64)1 << 28), ZKHIP_ERR_BAD_ARG, "count too large");
        ops_for(vk->curve)->verify(ctx, vk, count, proofs, inputs, ok_out);
    });
}
int32_t zkhip_verify_g16_batch(zkhip_ctx* ctx, const zkhip_vk* vk, uint64_t count, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out) {
    return verify_batch(ctx, vk, 0, count, proofs, inputs, ok_out);
}
int32_t zkhip_verify_gm17_batch(zkhip_ctx* ctx, const zkhip_vk* vk, uint64_t count, const uint8_t* proofs, const uint8_t* inputs, uint8_t* ok_out) {
    return verify_batch(ctx, vk, 1, count, proofs, inputs, ok_out);
}
int32_t zkhip_tower_op(zkhip_ctx* ctx, int32_t curve, int32_t op, uint64_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    return guarded_verify(ctx, [&] {
        const CurveOps* ops = ops_for(curve);
        require(op >= 0 && op < TOWER_OPS, ZKHIP_ERR_BAD_ARG, "unknown tower operation");
        if (count == 0) return;
        require(a && b && out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(count <= ((u64)1 << 20), ZKHIP_ERR_BAD_ARG, "count too large");
        ops->tower_op(ctx, op, count, a, b, out);
    });
}

int32_t zkhip_setup_g16_size(const zkhip_r1cs* cs, uint64_t* pk_bytes) {
    if (!cs || !pk_bytes) return ZKHIP_ERR_BAD_ARG;
    const u64 fqb = cs->curve == ZKHIP_CURVE_BN128 ? 32 : 48;
    const u64 g1 = 2 * fqb, g2 = 4 * fqb, m = cs->l + cs->w;
    *pk_bytes = g1 + 3 * g2 + 8 + cs->l * g1 + 2 * g1 + 8 + m * g1 + 8 + m * g1 + 8 + m * g2 + 8 + (cs->N - 1) * g1 + 8 + cs->w * g1;
    return ZKHIP_OK;
}
int32_t zkhip_setup_g16(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* toxic, const uint8_t* g1, const uint8_t* g2, uint8_t* pk_out,
                        uint64_t pk_cap) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && toxic && pk_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        ops_for(r1cs->curve)->setup(ctx, r1cs, toxic, g1, g2, pk_out, pk_cap);
    });
}

// ------------------------------------------------------------------ ZoKrates' own files (N1): host only, no context
int32_t zkhip_prog_parse(const uint8_t* bytes, size_t len, zkhip_prog** out) {
    if (!bytes || !out) { g_create_err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    *out = nullptr;
    return guarded_host([&] {
        std::unique_ptr<zkhip_prog> p(new zkhip_prog());
        prog_parse(bytes, len, p.get());
        *out = p.release();
    });
}
void zkhip_prog_free(zkhip_prog* prog) { delete prog; }
int32_t zkhip_prog_dims(const zkhip_prog* prog, uint64_t out[8]) {
    if (!prog || !out) return ZKHIP_ERR_BAD_ARG;
    out[0] = (uint64_t)prog->curve; out[1] = prog->n; out[2] = prog->l; out[3] = prog->w; out[4] = prog->return_count;
    out[5] = prog->public_args.size(); out[6] = prog->col[0].size() + prog->col[1].size() + prog->col[2].size(); out[7] = 0;
    return ZKHIP_OK;
}
int32_t zkhip_prog_matrix(const zkhip_prog* prog, int32_t which, const uint64_t** rowptr, const uint32_t** col, const uint8_t** val) {
    if (!prog || which < 0 || which > 2 || !rowptr || !col || !val) return ZKHIP_ERR_BAD_ARG;
    *rowptr = prog->rp[which].data();
    *col = prog->col[which].data();
    *val = prog->val[which].data();
    return ZKHIP_OK;
}
int32_t zkhip_prog_variable_order(const zkhip_prog* prog, const int64_t** ids) {
    if (!prog || !ids) return ZKHIP_ERR_BAD_ARG;
    *ids = prog->order.data();
    return ZKHIP_OK;
}
int32_t zkhip_prog_assignment(const zkhip_prog* prog, const uint8_t* witness, size_t len, uint8_t* z_out, uint8_t* inputs_out, uint64_t inputs_cap,
                              uint64_t* n_inputs) {
    if (!prog || !witness) { g_create_err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    return guarded_host([&] { prog_assignment(prog, witness, len, z_out, inputs_out, inputs_cap, n_inputs); });
}
int32_t zkhip_prog_write_bound(uint64_t n, uint64_t nnz, uint64_t n_args, uint64_t* bytes) {
    if (!bytes) return ZKHIP_ERR_BAD_ARG;
    *bytes = prog_write_bound(n, nnz, n_args);
    return ZKHIP_OK;
}
int32_t zkhip_prog_write(int32_t curve, uint64_t n, uint64_t m, const uint64_t* rowptr_a, const uint32_t* col_a, const uint8_t* val_a,
                         const uint64_t* rowptr_b, const uint32_t* col_b, const uint8_t* val_b, const uint64_t* rowptr_c, const uint32_t* col_c,
                         const uint8_t* val_c, const int64_t* ids, const int64_t* arg_ids, const uint8_t* arg_private, uint64_t n_args,
                         uint32_t return_count, uint8_t* out, uint64_t cap, uint64_t* len) {
    if (!rowptr_a || !rowptr_b || !rowptr_c || !ids || !out || !len || (n_args && (!arg_ids || !arg_private))) {
        g_create_err = "null argument";
        return ZKHIP_ERR_BAD_ARG;
    }
    return guarded_host([&] {
        const u64* rp[3] = {rowptr_a, rowptr_b, rowptr_c};
        const u32* col[3] = {col_a, col_b, col_c};
        const uint8_t* val[3] = {val_a, val_b, val_c};
        *len = prog_write(curve, n, m, rp, col, val, ids, arg_ids, arg_private, n_args, return_count, out, cap);
    });
}
int32_t zkhip_prog_r1cs_load(zkhip_ctx* ctx, const zkhip_prog* prog, zkhip_r1cs** out) {
    if (!ctx || !prog) return ZKHIP_ERR_BAD_ARG;
    return zkhip_r1cs_load(ctx, prog->curve, prog->n, prog->l, prog->w, prog->rp[0].data(), prog->col[0].data(), prog->val[0].data(),
                           prog->rp[1].data(), prog->col[1].data(), prog->val[1].data(), prog->rp[2].data(), prog->col[2].data(),
                           prog->val[2].data(), out);
}

// ------------------------------------------------------------------ N2: device-layout image of a loaded key (core.cuh PkImageHeader)
int32_t zkhip_pk_export_size(const zkhip_pk* pk, uint64_t* bytes) {
    if (!pk || !bytes) return ZKHIP_ERR_BAD_ARG;
    *bytes = ops_for(pk->curve)->pk_export_size(pk);
    return ZKHIP_OK;
}
int32_t zkhip_pk_export(const zkhip_pk* pk, uint8_t* out, uint64_t cap) {
    if (!pk || !out) return ZKHIP_ERR_BAD_ARG;
    return guarded(pk->ctx, [&] { ops_for(pk->curve)->pk_export(const_cast<zkhip_pk*>(pk), out, cap); });
}
int32_t zkhip_pk_import(zkhip_ctx* ctx, const uint8_t* bytes, size_t len, zkhip_pk** out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(bytes && out, ZKHIP_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        require(len >= sizeof(PkImageHeader), ZKHIP_ERR_PARSE, "key image truncated");
        PkImageHeader h;
        memcpy(&h, bytes, sizeof(h));
        require(!memcmp(h.magic, PK_IMAGE_MAGIC, 8), ZKHIP_ERR_PARSE, "not a key image of this library version (re-import the proving key)");
        const CurveOps* ops = ops_for(h.curve);   // (validates the curve id)
        std::unique_ptr<zkhip_pk> pk(new zkhip_pk());
        pk->curve = h.curve;
        pk->ctx = ctx;
        ops->pk_import(ctx, bytes, len, pk.get());
        *out = pk.release();
    });
}

// ------------------------------------------------------------------ one proof across several GPUs of one process
struct zkhip_multi {
    std::vector<zkhip_ctx*> ctx;     // one per member; a device may appear more than once
    std::vector<zkhip_pk*> pk;       // member k: shard k of n
    std::vector<zkhip_r1cs*> cs;     // replicas
    int scheme = -1;                 // of the loaded key: 0 Groth16, 1 GM17
    bool replicas = false;           // every member holds the WHOLE key (throughput mode) instead of shard k of n
    bool transform_split = true;     // bound members split the witness map (even members transform a, odd ones b, partners exchange)
    std::string err;
    // the exchange step over RCCL (zkhip_multi_use_rccl): one communicator and one pair of device buffers per member
    bool rccl = false;
    std::vector<void*> comm;         // ncclComm_t per member
    std::vector<DBuf> gather1, gather2;   // all members' ws1 / ws2, rank-major, on every member's device
    std::string rccl_desc;
    bool last_split = false;         // the last zkhip_prove_*_multi split its witness map
    bool transform_shard = false;    // unbound Groth16 proofs shard their witness map's domain across the members (zkhip_multi_transform_shard)
    int last_shard = 0;              // members the transforms of the last zkhip_multi_ntt / _witness_map / zkhip_prove_*_multi were sharded over
};
}  // extern "C"

// ------------------------------------------------------------------ RCCL, bound at run time
// The data path of a sharded proof has ONE exchange: every member contributes the bucket-set sums of its five partial
// MSMs ("ncclAllGather of a fixed-size struct").  libzkhip does not link librccl — a single-GPU prover, the
// CLI, the tests never need it and would pay its load time — so the five entry points used are resolved with dlopen when a
// caller asks for the RCCL exchange.  Whatever HIP runtime this process already runs is the one librccl.so.1 binds to.
#ifndef ZK_EMU
namespace {
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    std::string why;                 // why it is unavailable
};
Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            x.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (x.handle) break;
        }
        if (!x.handle) { x.why = std::string("librccl not loadable: ") + (dlerror() ? dlerror() : "?"); return x; }
        auto sym = [&](const char* n) { void* p = dlsym(x.handle, n); if (!p && x.why.empty()) x.why = std::string("librccl lacks ") + n; return p; };
        x.CommInitAll = (decltype(x.CommInitAll))sym("ncclCommInitAll");
        x.CommDestroy = (decltype(x.CommDestroy))sym("ncclCommDestroy");
        x.AllGather = (decltype(x.AllGather))sym("ncclAllGather");
        x.GroupStart = (decltype(x.GroupStart))sym("ncclGroupStart");
        x.GroupEnd = (decltype(x.GroupEnd))sym("ncclGroupEnd");
        x.GetErrorString = (decltype(x.GetErrorString))sym("ncclGetErrorString");
        x.GetVersion = (decltype(x.GetVersion))sym("ncclGetVersion");
        return x;
    }();
    return r;
}
void rccl_check(ncclResult_t rc, const char* what) {
    if (rc != ncclSuccess) throw DevError{std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(rc) : "RCCL error")};
}
}  // namespace
#endif
// run fn(k) for every member — one host thread each (contexts are independent; the test emulator is single-threaded) —
// and keep the first failure
template <class Fn>
static int32_t multi_each(zkhip_multi* m, Fn&& fn) try {
    const size_t n = m->ctx.size();
    std::vector<int32_t> rc(n, ZKHIP_OK);
    std::vector<std::string> msg(n);
    auto body = [&](size_t k) {
        rc[k] = fn(k);
        if (rc[k] != ZKHIP_OK) msg[k] = zkhip_last_error(m->ctx[k]);
    };
#ifdef ZK_EMU
    for (size_t k = 0; k < n; ++k) body(k);
#else
    {
        HostThreads th;
        for (size_t k = 1; k < n; ++k) th.run([&, k] { body(k); });
        body(0);
    }
#endif
    for (size_t k = 0; k < n; ++k)
        if (rc[k] != ZKHIP_OK) {
            m->err = "member " + std::to_string(k) + ": " + msg[k];
            return rc[k];
        }
    return ZKHIP_OK;
} catch (const std::bad_alloc&) {   // nothing may escape through the C ABI (HostThreads joins what was started)
    return ZKHIP_ERR_NOMEM;
} catch (...) {
    return ZKHIP_ERR_DEVICE;
}
// every member holds a constraint system and a key
static bool multi_loaded(const zkhip_multi* m) {
    for (auto* c : m->cs) if (!c) return false;
    for (auto* p : m->pk) if (!p) return false;
    return true;
}
// fn(k) on every member: the plan's split where member k can shard, -1 where it cannot.  Sharded only if all agree.
template <class Fn>
static bool multi_all_shard(zkhip_multi* m, Fn&& fn) {
    const size_t n = m->ctx.size();
    if (n < 2) return false;
    int first = -1;
    for (size_t k = 0; k < n; ++k) {
        int v = -1;
        if (guarded(m->ctx[k], [&] { v = fn(k); }) != ZKHIP_OK || v < 0 || (k && v != first)) return false;
        first = v;
    }
    return true;
}
extern "C" {
static void multi_drop_keys(zkhip_multi* m) {
    for (auto*& p : m->pk) { zkhip_pk_free(p); p = nullptr; }
    m->scheme = -1;
    m->replicas = false;
}
int32_t zkhip_ctx_create_multi(const int32_t* devices, int32_t n, zkhip_multi** out) {
    if (!out) { g_create_err = "out is NULL"; return ZKHIP_ERR_BAD_ARG; }
    *out = nullptr;
    if (!devices || n < 1 || n > 64) { g_create_err = "device list empty or longer than 64"; return ZKHIP_ERR_BAD_ARG; }
    std::unique_ptr<zkhip_multi> m(new (std::nothrow) zkhip_multi());
    if (!m) { g_create_err = "out of host memory"; return ZKHIP_ERR_NOMEM; }
    try {
        m->ctx.reserve(n);
        m->pk.assign(n, nullptr);
        m->cs.assign(n, nullptr);
    } catch (const std::bad_alloc&) {
        g_create_err = "out of host memory";
        return ZKHIP_ERR_NOMEM;
    }
    for (int32_t k = 0; k < n; ++k) {
        zkhip_ctx* c = nullptr;
        const int32_t rc = zkhip_ctx_create(devices[k], &c);
        if (rc != ZKHIP_OK) {
            for (auto* q : m->ctx) zkhip_ctx_free(q);
            return rc;        // message already in the per-thread create error
        }
        m->ctx.push_back(c);  // (capacity reserved above)
    }
    // members that share a device share its memory: each sizes its tables for its share of what is free (msm_table_budget)
    for (int32_t k = 0; k < n; ++k) {
        int same = 0;
        for (int32_t q = 0; q < n; ++q) same += devices[q] == devices[k];
        m->ctx[k]->tenants = same;
    }
    *out = m.release();
    return ZKHIP_OK;
}
static void multi_drop_rccl(zkhip_multi* m) {
#ifndef ZK_EMU
    for (size_t k = 0; k < m->comm.size(); ++k)
        if (m->comm[k]) {
            try { dev_set(m->ctx[k]->device); } catch (...) {}
            (void)rccl().CommDestroy((ncclComm_t)m->comm[k]);
        }
#endif
    m->comm.clear();
    for (size_t k = 0; k < m->gather1.size(); ++k) {
        try { dev_set(m->ctx[k]->device); } catch (...) {}
        m->gather1[k].release();
        m->gather2[k].release();
    }
    m->gather1.clear();
    m->gather2.clear();
    m->rccl = false;
}
int32_t zkhip_multi_use_rccl(zkhip_multi* m, int32_t on) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    try {
        multi_drop_rccl(m);
        if (!on) return ZKHIP_OK;
        const size_t n = m->ctx.size();
        std::vector<int> dev(n);
        for (size_t k = 0; k < n; ++k) dev[k] = m->ctx[k]->device;
#ifndef ZK_EMU   // (the emulator's "all-gather" is a loop of copies: its members may share the one emulated device)
        for (size_t a = 0; a < n; ++a)
            for (size_t b = a + 1; b < n; ++b)
                if (dev[a] == dev[b]) {
                    m->err = "RCCL wants one device per member (device " + std::to_string(dev[a]) + " is listed twice): the host exchange stays in use";
                    return ZKHIP_ERR_BAD_ARG;
                }
#endif
        m->gather1 = std::vector<DBuf>(n);
        m->gather2 = std::vector<DBuf>(n);
#ifdef ZK_EMU
        m->rccl_desc = "emulated all-gather (TEST EMULATOR: device-to-device copies in member order)";
#else
        Rccl& R = rccl();
        if (!R.why.empty()) { m->err = R.why; m->gather1.clear(); m->gather2.clear(); return ZKHIP_ERR_DEVICE; }
        std::vector<ncclComm_t> comms(n, nullptr);
        rccl_check(R.CommInitAll(comms.data(), (int)n, dev.data()), "ncclCommInitAll");
        m->comm.assign(comms.begin(), comms.end());
        int ver = 0;
        (void)R.GetVersion(&ver);
        m->rccl_desc = "RCCL " + std::to_string(ver) + ", " + std::to_string(n) + " rank(s), ncclAllGather of the members' bucket-set sums";
        for (size_t a = 0; a < n; ++a)          // xGMI peer reachability, for the record (RCCL picks its own transport)
            for (size_t b = 0; b < n; ++b) {
                int can = 0;
                if (a != b && hipDeviceCanAccessPeer(&can, dev[a], dev[b]) == hipSuccess && !can) m->rccl_desc += "; no peer access " + std::to_string(dev[a]) + "->" + std::to_string(dev[b]);
            }
#endif
        m->rccl = true;
        return ZKHIP_OK;
    } catch (const DevError& e) {
        m->err = e.msg;
        multi_drop_rccl(m);
        return ZKHIP_ERR_DEVICE;
    } catch (const std::bad_alloc&) {
        m->err = "out of host memory";
        multi_drop_rccl(m);
        return ZKHIP_ERR_NOMEM;
    } catch (...) {
        m->err = "unexpected internal error";
        multi_drop_rccl(m);
        return ZKHIP_ERR_DEVICE;
    }
}
const char* zkhip_multi_exchange(const zkhip_multi* m) {
    if (!m) return "";
    return m->rccl ? m->rccl_desc.c_str() : "canonical records in host memory, combined on the calling thread";
}
void zkhip_multi_free(zkhip_multi* m) {
    if (!m) return;
    multi_drop_rccl(m);
    multi_drop_keys(m);
    for (auto* c : m->cs) zkhip_r1cs_free(c);
    for (auto* c : m->ctx) zkhip_ctx_free(c);
    delete m;
}
int32_t zkhip_multi_size(const zkhip_multi* m) { return m ? (int32_t)m->ctx.size() : 0; }
zkhip_ctx* zkhip_multi_ctx(zkhip_multi* m, int32_t member) { return (m && member >= 0 && (size_t)member < m->ctx.size()) ? m->ctx[member] : nullptr; }
const char* zkhip_multi_last_error(const zkhip_multi* m) { return m ? m->err.c_str() : g_create_err.c_str(); }
int32_t zkhip_multi_r1cs_load(zkhip_multi* m, int32_t curve, uint64_t n, uint64_t l, uint64_t w, const uint64_t* rowptr_a, const uint32_t* col_a,
                              const uint8_t* val_a, const uint64_t* rowptr_b, const uint32_t* col_b, const uint8_t* val_b, const uint64_t* rowptr_c,
                              const uint32_t* col_c, const uint8_t* val_c) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    auto drop = [&] { for (auto*& c : m->cs) { zkhip_r1cs_free(c); c = nullptr; } };
    drop();
    const int32_t rc = multi_each(m, [&](size_t k) {
        return zkhip_r1cs_load(m->ctx[k], curve, n, l, w, rowptr_a, col_a, val_a, rowptr_b, col_b, val_b, rowptr_c, col_c, val_c, &m->cs[k]);
    });
    if (rc != ZKHIP_OK) drop();      // all members or none: a partly loaded group must not reach the provers
    return rc;
}
// member k: shard k of n of the key, or — `replicas` — the whole key
static int32_t multi_load(zkhip_multi* m, int32_t curve, int scheme, bool replicas, const uint8_t* bytes, size_t len) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    multi_drop_keys(m);
    const uint32_t world = replicas ? 1 : (uint32_t)m->ctx.size();
    const int32_t rc = multi_each(m, [&](size_t k) { return load_key(m->ctx[k], curve, scheme, bytes, len, replicas ? 0 : (uint32_t)k, world, &m->pk[k]); });
    if (rc == ZKHIP_OK) { m->scheme = scheme; m->replicas = replicas; } else multi_drop_keys(m);
    return rc;
}
int32_t zkhip_multi_pk_load_g16(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len) { return multi_load(m, curve, 0, false, bytes, len); }
int32_t zkhip_multi_pk_load_gm17(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len) { return multi_load(m, curve, 1, false, bytes, len); }
// throughput mode: the whole key on every member; zkhip_prove_g16_multi_batch deals independent proofs round-robin
int32_t zkhip_multi_pk_load_g16_replicas(zkhip_multi* m, int32_t curve, const uint8_t* bytes, size_t len) { return multi_load(m, curve, 0, true, bytes, len); }
// The members' keys bound to the members' constraint system: member 0 computes level 0 of H' / L' over the whole index range from
// the key file (the same bytes the key was loaded from), every member installs its own ranges (replicas: all of it).
int32_t zkhip_multi_bind(zkhip_multi* m, const uint8_t* key_bytes, size_t len) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    if (!key_bytes) { m->err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    if (m->scheme < 0 || !multi_loaded(m)) { m->err = "load the constraint system and a proving key first"; return ZKHIP_ERR_BAD_ARG; }
    std::vector<uint8_t> h_host, l_host;
    u64 fp[2] = {0, 0};
    const CurveOps* ops = nullptr;
    int32_t rc = guarded(m->ctx[0], [&] {
        ops = ops_for(m->pk[0]->curve);
        for (size_t k = 0; k < m->ctx.size(); ++k) ops->pk_bind_check(m->ctx[k], m->pk[k], m->cs[k]);
        ops->bound_level0_from_file(m->ctx[0], m->scheme, m->cs[0], key_bytes, len, h_host, l_host, fp);
    });
    if (rc != ZKHIP_OK) { m->err = std::string("member 0: ") + zkhip_last_error(m->ctx[0]); return rc; }
    rc = multi_each(m, [&](size_t k) {
        return guarded(m->ctx[k], [&] { ops->install_bound_ranges(m->ctx[k], m->pk[k], m->cs[k], h_host.data(), h_host.size(), l_host.data(), l_host.size(), fp); });
    });
    if (rc != ZKHIP_OK) for (auto* p : m->pk) zkhip_pk_unbind(p);      // all members or none
    return rc;
}
// 1 / 0: let bound members split the witness map of a proof between them (default 1); returns what it was.  -1: only report.
int32_t zkhip_multi_transform_split(zkhip_multi* m, int32_t on) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    const int32_t was = m->transform_split ? 1 : 0;
    if (on >= 0) m->transform_split = on != 0;
    return was;
}
// 1 if the last zkhip_prove_*_multi split its witness map between the members, else 0
int32_t zkhip_multi_last_split(const zkhip_multi* m) { return m && m->last_split ? 1 : 0; }
int32_t zkhip_multi_unbind(zkhip_multi* m) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    for (auto* p : m->pk) if (p) zkhip_pk_unbind(p);
    return ZKHIP_OK;
}
int32_t zkhip_prove_g16_multi_batch(zkhip_multi* m, uint32_t count, const uint8_t* z, const uint8_t* rs, uint8_t* proofs_out, zkhip_timings* timings) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    if ((!z || !rs || !proofs_out) && count) { m->err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    if (m->scheme != 0 || !m->replicas || !multi_loaded(m)) {
        m->err = "load the constraint system and zkhip_multi_pk_load_g16_replicas first";
        return ZKHIP_ERR_BAD_ARG;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = m->ctx.size();
    const uint64_t zb = (uint64_t)m->pk[0]->m * 32;
    const size_t proof_bytes = (m->pk[0]->curve == ZKHIP_CURVE_BN128 ? 32 : 48) * 8 + 3;
    // member k proves the contiguous block [lo_k, hi_k) of the batch through its own pipelined batch call
    std::vector<zkhip_timings> tm(n);
    const int32_t rc = multi_each(m, [&](size_t k) {
        const uint64_t lo = (uint64_t)count * k / n, hi = (uint64_t)count * (k + 1) / n;
        memset(&tm[k], 0, sizeof(tm[k]));
        if (hi == lo) return (int32_t)ZKHIP_OK;
        return zkhip_prove_g16_batch(m->ctx[k], m->pk[k], m->cs[k], (uint32_t)(hi - lo), z + lo * zb, rs + lo * 64, proofs_out + lo * proof_bytes, &tm[k]);
    });
    if (rc != ZKHIP_OK) return rc;
    if (timings) {
        memset(timings, 0, sizeof(*timings));
        for (size_t k = 0; k < n; ++k) {
            float* a = (float*)timings; const float* b = (const float*)&tm[k];
            for (size_t q = 0; q < sizeof(zkhip_timings) / sizeof(float); ++q) a[q] += b[q];
        }
        timings->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return ZKHIP_OK;
}
static void multi_split_drop(zkhip_multi* m) {
    for (auto* c : m->ctx) split_drop(c);
}
// ---- transforms sharded across the members (ntt_shard.h): every step runs on every member before the next step on any — a
// member fetches what its peers packed in the step before — and a failure in any step drops every member: nothing stays pending, no
// staging turn is left half taken, and nobody waits for an event that will never be recorded
static void multi_shard_drop(zkhip_multi* m) {
    for (auto* c : m->ctx) {
        try { dev_set(c->device); dev_sync_all(); } catch (...) {}
        c->shard.turn = 0;
        split_drop(c);
    }
}
int32_t zkhip_multi_transform_shard(zkhip_multi* m, int32_t on) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    const int32_t was = m->transform_shard ? 1 : 0;
    if (on >= 0) m->transform_shard = on != 0;
    return was;
}
int32_t zkhip_multi_last_shard(const zkhip_multi* m) { return m ? m->last_shard : 0; }
int32_t zkhip_multi_ntt(zkhip_multi* m, int32_t curve, uint32_t log_n, int32_t dir, uint8_t* data) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    m->last_shard = 0;
    const CurveOps* ops = nullptr;
    int32_t rc = guarded(m->ctx[0], [&] {
        require(data && dir >= 0 && dir <= 3, ZKHIP_ERR_BAD_ARG, "bad argument");
        ops = ops_for(curve);
    });
    if (rc != ZKHIP_OK) { m->err = std::string("member 0: ") + zkhip_last_error(m->ctx[0]); return rc; }
    const uint32_t n = (uint32_t)m->ctx.size();
    if (!multi_all_shard(m, [&](size_t k) { return ops->ntt_shardable(m->ctx[k], log_n, n); })) {
        rc = zkhip_ntt(m->ctx[0], curve, log_n, dir, data);      // not shardable: the single-context transform on member 0
        if (rc != ZKHIP_OK) m->err = std::string("member 0: ") + zkhip_last_error(m->ctx[0]);
        return rc;
    }
    // (in place: every member has read its strip of `data` before any member writes its part of the result)
    rc = multi_each(m, [&](size_t k) { return guarded(m->ctx[k], [&] { ops->shard_ntt_begin(m->ctx[k], n, (uint32_t)k, log_n, dir, data); }); });
    if (rc == ZKHIP_OK)
        rc = multi_each(m, [&](size_t k) { return guarded(m->ctx[k], [&] { ops->shard_ntt_end(m->ctx[k], n, (uint32_t)k, log_n, dir, data, m->ctx.data()); }); });
    if (rc != ZKHIP_OK) { multi_shard_drop(m); return rc; }
    m->last_shard = (int)n;
    return ZKHIP_OK;
}
int32_t zkhip_multi_witness_map(zkhip_multi* m, const uint8_t* z, uint8_t* h_out) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    m->last_shard = 0;
    if (!z || !h_out) { m->err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    for (auto* c : m->cs) if (!c) { m->err = "load the constraint system first"; return ZKHIP_ERR_BAD_ARG; }
    const CurveOps* ops = nullptr;
    int32_t rc = guarded(m->ctx[0], [&] { ops = ops_for(m->cs[0]->curve); });
    if (rc != ZKHIP_OK) { m->err = std::string("member 0: ") + zkhip_last_error(m->ctx[0]); return rc; }
    const uint32_t n = (uint32_t)m->ctx.size();
    if (!multi_all_shard(m, [&](size_t k) { return ops->witness_map_shardable(m->ctx[k], m->cs[k], n); })) {
        rc = zkhip_witness_map(m->ctx[0], m->cs[0], z, h_out);
        if (rc != ZKHIP_OK) m->err = std::string("member 0: ") + zkhip_last_error(m->ctx[0]);
        return rc;
    }
    for (int step = 0; step < 4; ++step) {
        rc = multi_each(m, [&](size_t k) {
            return guarded(m->ctx[k], [&] { ops->shard_witness_map(m->ctx[k], m->cs[k], z, h_out, n, (uint32_t)k, step, m->ctx.data()); });
        });
        if (rc != ZKHIP_OK) { multi_shard_drop(m); return rc; }
    }
    m->last_shard = (int)n;
    return ZKHIP_OK;
}
static int32_t multi_prove(zkhip_multi* m, int scheme, const uint8_t* z, const uint8_t* rnd, const uint8_t* s_, uint8_t* proof_out, zkhip_timings* timings) {
    if (!m) return ZKHIP_ERR_BAD_ARG;
    if (!z || !rnd || !proof_out || (scheme == 0 && !s_)) { m->err = "null argument"; return ZKHIP_ERR_BAD_ARG; }
    if (m->scheme != scheme || !multi_loaded(m)) { m->err = "load the constraint system and a proving key of this scheme first"; return ZKHIP_ERR_BAD_ARG; }
    if (m->replicas) { m->err = "the members hold whole keys (replicas): use zkhip_prove_g16_multi_batch, or load the key sharded"; return ZKHIP_ERR_BAD_ARG; }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t rec = 0;
    zkhip_partial_size(m->pk[0]->curve, &rec);
    const size_t n = m->ctx.size();
    std::vector<uint8_t> records(n * rec);
    std::vector<zkhip_timings> tm(n);
    int32_t rc;
    // The witness map SPLIT between the members (SURVEY.md §8e / north_star "NTT domain shard"): over keys bound to the system a proof
    // needs a and b on the coset and nothing else — members of even rank transform a, those of odd rank b (two transforms instead
    // of four each), partners copy each other's vector (N x 32 B over xGMI, or on the device they share) and every member multiplies.
    // Unbound keys, GM17, one member, domains below 2^18: every member runs the whole map, as before.
    const CurveOps* sops = ops_for(m->pk[0]->curve);
    bool split = scheme == 0 && n >= 2 && m->transform_split;
    for (size_t k = 0; k < n && split; ++k) split = sops->can_split(m->ctx[k], m->pk[k], m->cs[k]);
    auto half_of = [](size_t k) { return (int)(k & 1); };
    auto partner_of = [n](size_t k) { return (k ^ 1) < n ? (k ^ 1) : k - 1; };
    auto fetch = [&](size_t k) {      // (inside guarded(m->ctx[k], ...))
        const size_t p = partner_of(k);
        sops->split_fetch(m->ctx[k], m->pk[k], sops->split_half_ptr(m->ctx[p], m->pk[p], half_of(p)), m->ctx[p]->device, m->ctx[p]->slots[0].half_ready);
    };
    m->last_split = split;
    // ... or its DOMAIN sharded across them (zkhip_multi_transform_shard; ntt_shard.h): an unbound Groth16 key, a power-of-two member
    // count the plan divides by, every member's h range the range the sharded last transform leaves its h coefficients in.  Bound keys
    // keep the split above; GM17 and whatever does not shard stay replicated.  The first three of shard_witness_map's four steps run
    // here, each on every member before the next on any; the fourth leads a member's tail below.
    const uint32_t G = (uint32_t)n;
    const bool shard = !split && scheme == 0 && m->transform_shard && multi_all_shard(m, [&](size_t k) { return sops->can_shard(m->ctx[k], m->pk[k], m->cs[k], G, (uint32_t)k); });
    m->last_shard = shard ? (int)n : 0;
    if (shard) {
        rc = multi_each(m, [&](size_t k) {
            return guarded(m->ctx[k], [&] {
                require(m->pk[k]->ctx == m->ctx[k] && m->cs[k]->ctx == m->ctx[k], ZKHIP_ERR_BAD_ARG, "handles belong to another context");
                for (auto& sl : m->ctx[k]->slots) require(!sl.busy, ZKHIP_ERR_BAD_ARG, "a proof is in flight in this context");
                sops->shard_begin(m->ctx[k], m->pk[k], m->cs[k], z, rnd, s_, G, (uint32_t)k);
            });
        });
        for (int step = 1; step <= 2 && rc == ZKHIP_OK; ++step)
            rc = multi_each(m, [&](size_t k) {
                return guarded(m->ctx[k], [&] { sops->shard_step(m->ctx[k], m->pk[k], m->cs[k], G, (uint32_t)k, step, m->ctx.data()); }, true);
            });
        if (rc != ZKHIP_OK) { multi_shard_drop(m); return rc; }
    }
    auto shard_last = [&](size_t k) { sops->shard_step(m->ctx[k], m->pk[k], m->cs[k], G, (uint32_t)k, 3, m->ctx.data()); };
    auto drop = [&] { if (shard) multi_shard_drop(m); else multi_split_drop(m); };
    if (split) {
        // phase A on every member before phase B on any: a member fetches its partner's half only when that half is enqueued
        rc = multi_each(m, [&](size_t k) {
            return guarded(m->ctx[k], [&] {
                require(m->pk[k]->ctx == m->ctx[k] && m->cs[k]->ctx == m->ctx[k], ZKHIP_ERR_BAD_ARG, "handles belong to another context");
                for (auto& sl : m->ctx[k]->slots) require(!sl.busy, ZKHIP_ERR_BAD_ARG, "a proof is in flight in this context");
                sops->split_begin(m->ctx[k], m->pk[k], m->cs[k], z, nullptr, rnd, s_, half_of(k));
            });
        });
        if (rc != ZKHIP_OK) { multi_split_drop(m); return rc; }      // (no member stays pending behind another member's failure)
    }
    if (m->rccl) {
        // every member leaves the bucket-set sums of its five partial MSMs on its device and all-gathers them (RCCL over
        // xGMI; in the test emulator: copies in member order); member 0's gathered copy is read back and combined
        const CurveOps* ops = ops_for(m->pk[0]->curve);
        std::vector<const void*> d1(n), d2(n);
        std::vector<size_t> b1(n), b2(n);
        auto share = [&](size_t k) {
            return guarded(m->ctx[k], [&] {
                zkhip_ctx* c = m->ctx[k];
                require(m->pk[k]->ctx == c && m->cs[k]->ctx == c, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
                if (split) { fetch(k); ops->split_end_device_sums(c, m->pk[k], m->cs[k], &d1[k], &b1[k], &d2[k], &b2[k], &tm[k]); }
                else if (shard) { shard_last(k); ops->shard_end_device_sums(c, m->pk[k], m->cs[k], &d1[k], &b1[k], &d2[k], &b2[k], &tm[k]); }
                else if (scheme == 0) ops->prove_device_sums(c, m->pk[k], m->cs[k], z, rnd, s_, &d1[k], &b1[k], &d2[k], &b2[k], &tm[k]);
                else ops->gm17_prove_device_sums(c, m->pk[k], m->cs[k], z, rnd, &d1[k], &b1[k], &d2[k], &b2[k], &tm[k]);
                m->gather1[k].ensure(n * b1[k]);
                m->gather2[k].ensure(n * b2[k]);
            }, split || shard);
        };
#ifdef ZK_EMU
        rc = multi_each(m, share);
        if (rc != ZKHIP_OK) { drop(); return rc; }
        for (size_t k = 0; k < n; ++k) {
            dev_d2d((uint8_t*)m->gather1[0].p + k * b1[0], d1[k], b1[0], m->ctx[0]->stream);
            dev_d2d((uint8_t*)m->gather2[0].p + k * b2[0], d2[k], b2[0], m->ctx[0]->stream);
        }
#else
        // two phases: a member enters the collective only when EVERY member has its share (one that failed alone would
        // leave the others waiting in ncclAllGather for ever)
        rc = multi_each(m, share);
        if (rc != ZKHIP_OK) { drop(); return rc; }
        rc = multi_each(m, [&](size_t k) {
            return guarded(m->ctx[k], [&] {
                Rccl& R = rccl();
                zkhip_ctx* c = m->ctx[k];
                rccl_check(R.GroupStart(), "ncclGroupStart");
                rccl_check(R.AllGather(d1[k], m->gather1[k].p, b1[k], ncclUint8, (ncclComm_t)m->comm[k], c->stream), "ncclAllGather");
                rccl_check(R.AllGather(d2[k], m->gather2[k].p, b2[k], ncclUint8, (ncclComm_t)m->comm[k], c->stream), "ncclAllGather");
                rccl_check(R.GroupEnd(), "ncclGroupEnd");
                stream_sync(c->stream);
            });
        });
        if (rc != ZKHIP_OK) return rc;
#endif
        rc = guarded(m->ctx[0], [&] {
            std::vector<uint8_t> h1(n * b1[0]), h2(n * b2[0]);
            dev_d2h(h1.data(), m->gather1[0].p, h1.size(), m->ctx[0]->stream);
            dev_d2h(h2.data(), m->gather2[0].p, h2.size(), m->ctx[0]->stream);
            stream_sync(m->ctx[0]->stream);
            for (size_t k = 0; k < n; ++k) ops->record_from_sums(m->ctx[k], m->pk[k], &h1[k * b1[0]], &h2[k * b2[0]], &records[k * rec]);
        });
        if (rc != ZKHIP_OK) { m->err = std::string("gather: ") + zkhip_last_error(m->ctx[0]); return rc; }
    } else {
        rc = multi_each(m, [&](size_t k) {
            if (split) return guarded(m->ctx[k], [&] { fetch(k); sops->split_end_partial(m->ctx[k], m->pk[k], m->cs[k], &records[k * rec], &tm[k]); }, true);
            if (shard) return guarded(m->ctx[k], [&] { shard_last(k); sops->shard_end_partial(m->ctx[k], m->pk[k], m->cs[k], &records[k * rec], &tm[k]); }, true);
            return scheme == 0 ? zkhip_prove_g16_partial(m->ctx[k], m->pk[k], m->cs[k], z, nullptr, rnd, s_, &records[k * rec], &tm[k])
                               : zkhip_prove_gm17_partial(m->ctx[k], m->pk[k], m->cs[k], z, nullptr, rnd, &records[k * rec], &tm[k]);
        });
        if (rc != ZKHIP_OK) { drop(); return rc; }
    }
    rc = scheme == 0 ? zkhip_combine_g16(m->ctx[0], m->pk[0], (uint32_t)n, records.data(), rnd, s_, proof_out)
                     : zkhip_combine_gm17(m->ctx[0], m->pk[0], (uint32_t)n, records.data(), rnd, proof_out);
    if (rc != ZKHIP_OK) { m->err = std::string("combine: ") + zkhip_last_error(m->ctx[0]); return rc; }
    if (timings) {   // the slowest member per phase; total = wall clock of the whole call
        *timings = tm[0];
        for (size_t k = 1; k < n; ++k) {
            float* a = (float*)timings; const float* b = (const float*)&tm[k];
            for (size_t q = 0; q < sizeof(zkhip_timings) / sizeof(float); ++q) a[q] = std::max(a[q], b[q]);
        }
        timings->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return ZKHIP_OK;
}
int32_t zkhip_prove_g16_multi(zkhip_multi* m, const uint8_t* z, const uint8_t* r, const uint8_t* s, uint8_t* proof_out, zkhip_timings* timings) {
    return multi_prove(m, 0, z, r, s, proof_out, timings);
}
int32_t zkhip_prove_gm17_multi(zkhip_multi* m, const uint8_t* z, const uint8_t* d1_d2_r, uint8_t* proof_out, zkhip_timings* timings) {
    return multi_prove(m, 1, z, d1_d2_r, nullptr, proof_out, timings);
}

// ------------------------------------------------------------------ GM17 (config 5)
int32_t zkhip_prove_gm17_partial(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, zkhip_assignment* z_resident,
                                 const uint8_t* d1_d2_r, uint8_t* partial_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && (z || z_resident) && d1_d2_r && partial_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        if (!z) require(z_resident->ctx == ctx && z_resident->curve == pk->curve && z_resident->m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG,
                        "assignment does not match the constraint system");
        ops_for(pk->curve)->gm17_prove_partial(ctx, pk, r1cs, z, z ? nullptr : z_resident->scalars.p, d1_d2_r, partial_out, timings);
    });
}
int32_t zkhip_combine_gm17(zkhip_ctx* ctx, const zkhip_pk* pk, uint32_t count, const uint8_t* partials, const uint8_t* d1_d2_r, uint8_t* proof_out) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && partials && d1_d2_r && proof_out && count >= 1, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->scheme == 1, ZKHIP_ERR_BAD_ARG, "this is a Groth16 proving key");
        ops_for(pk->curve)->gm17_combine(pk, count, partials, d1_d2_r, proof_out);
    }, true);
}
int32_t zkhip_prove_gm17(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, const uint8_t* z, const uint8_t* d1_d2_r,
                         uint8_t* proof_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && z && d1_d2_r && proof_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        ops_for(pk->curve)->gm17_prove(ctx, pk, r1cs, z, nullptr, d1_d2_r, proof_out, timings);
    });
}
int32_t zkhip_prove_gm17_resident(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, zkhip_assignment* z, const uint8_t* d1_d2_r,
                                  uint8_t* proof_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && z && d1_d2_r && proof_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx && z->ctx == ctx, ZKHIP_ERR_BAD_ARG, "handles belong to another context");
        require(z->curve == pk->curve && z->m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG, "assignment does not match the constraint system");
        ops_for(pk->curve)->gm17_prove(ctx, pk, r1cs, nullptr, z->scalars.p, d1_d2_r, proof_out, timings);
    });
}
int32_t zkhip_prove_gm17_resident_batch(zkhip_ctx* ctx, const zkhip_pk* pk, const zkhip_r1cs* r1cs, uint32_t count, zkhip_assignment* const* zs,
                                        const uint8_t* d1_d2_r, uint8_t* proofs_out, zkhip_timings* timings) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(pk && r1cs && d1_d2_r && proofs_out && (zs || count == 0), ZKHIP_ERR_BAD_ARG, "null argument");
        require(pk->ctx == ctx && r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "key / constraint system belong to another context");
        std::vector<void*> dev(count);
        for (uint32_t i = 0; i < count; ++i) {
            require(zs[i] && zs[i]->ctx == ctx && zs[i]->curve == pk->curve && zs[i]->m == r1cs->l + r1cs->w, ZKHIP_ERR_BAD_ARG,
                    "assignment does not match the constraint system");
            dev[i] = zs[i]->scalars.p;
        }
        ops_for(pk->curve)->gm17_prove_batch(ctx, pk, r1cs, count, nullptr, dev.data(), d1_d2_r, proofs_out, timings);
    });
}
int32_t zkhip_setup_gm17_size(const zkhip_r1cs* cs, uint64_t* pk_bytes) {
    if (!cs || !pk_bytes) return ZKHIP_ERR_BAD_ARG;
    try {
        *pk_bytes = ops_for(cs->curve)->gm17_key_bytes(cs->n, cs->l, cs->w);
    } catch (...) {
        return ZKHIP_ERR_BAD_ARG;
    }
    return ZKHIP_OK;
}
int32_t zkhip_setup_gm17(zkhip_ctx* ctx, const zkhip_r1cs* r1cs, const uint8_t* toxic, const uint8_t* g1, const uint8_t* g2, uint8_t* pk_out,
                         uint64_t pk_cap) {
    if (!ctx) return ZKHIP_ERR_BAD_ARG;
    return guarded(ctx, [&] {
        require(r1cs && toxic && pk_out, ZKHIP_ERR_BAD_ARG, "null argument");
        require(r1cs->ctx == ctx, ZKHIP_ERR_BAD_ARG, "constraint system belongs to another context");
        ops_for(r1cs->curve)->gm17_setup(ctx, r1cs, toxic, g1, g2, pk_out, pk_cap);
    });
}

}  // extern "C"
