// wexec.cuh — the device side of witnesses computed on the device (include/zkhip.h "witnesses computed on the device"; the compile
// pass that writes the instruction stream is host code: xplan.h).  What `Interpreter::execute` does per proof on one host thread
// (/root/reference/zokrates_interpreter/src/lib.rs:30-138: walk the statements over a BTreeMap) a batch does here in one launch:
//   k_exec_program       one work-item per INSTANCE.  A program is a straight-line list and no control flow depends on a value, so
//                        every lane of a wave executes the same instruction: the stream is read at a wave-uniform address (scalar
//                        loads), and the values live in a store laid out [slot][instance of the chunk], 32 B each, Montgomery form —
//                        the 64 loads or stores of a wave's instruction are 2 KiB of consecutive bytes;
//   k_exec_level,        the level-scheduled route of the same call (ZKHIP_TUNE_EXEC_WIDE): one work-item per (instruction of a level,
//   k_exec_levels_run    instance) over the plan's dependency levels — a lone instance, or a few, across the device.  The same store, verdict
//                        words and opcode bodies (wx_step: one body per opcode, over words read uniformly or per lane);
//   k_exec_gather        slots -> canonical 32-byte integers: the z of every instance that ran through, into its own resident
//                        assignment (column j is slot j), and the public inputs;
//   k_exec_witness_file  the reference's `witness` bytes per instance: u64 count, then (i64 id, 32-byte LE value) by ascending id.
// Where lanes of one wave differ — a zero divisor, a failed check — nothing branches on the data: both outcomes are computed and one
// is selected, and a failing lane records the statement and carries on.  No per-lane array is indexed at run time (bits are taken limb
// by limb, each written straight to the store), so the main loop keeps its values in registers.
#pragma once
#include "devrt.h"
#include "field.cuh"
#include "xplan.h"

namespace zk {

static constexpr u32 WX_BLOCK = 64;                   // one wave per workgroup: the waves of a chunk spread over the compute units
static constexpr u32 WX_RAN_THROUGH = 0xffffffffu;    // an instance's verdict word when no check failed (else: the lowest failing statement)

// a word of the instruction stream: the same in every lane (the stream's address never depends on a lane), said so that the compiler
// keeps it — and every address and trip count made from it — in scalar registers
#if defined(__HIP_DEVICE_COMPILE__)
#define WX_UNIFORM(x) ((u32)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define WX_UNIFORM(x) ((u32)(x))
#endif
template <bool UNI>
__device__ __forceinline__ u32 wx_word(u32 x) {      // a word of the stream as a kernel reads it: uniform, or the lane's own
    if constexpr (UNI) return WX_UNIFORM(x);
    else return x;
}

template <class F>
__device__ __forceinline__ F wx_load(const F* p) {
    const uint4* __restrict__ q = (const uint4*)p;
    const uint4 a = q[0], b = q[1];
    F r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
template <class F>
__device__ __forceinline__ void wx_store(F* p, const F& x) {
    uint4* q = (uint4*)p;
    q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
template <class F>
__device__ __forceinline__ F wx_select(bool c, const F& a, const F& b) {      // c ? a : b, word by word
    F r;
    ZK_UNROLL for (int i = 0; i < F::N; ++i) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}
// a^(r - 2): the exponent is the modulus' own words, so every branch is the same in every lane (0 -> 0).  Inline, its operands in
// registers: the library's fe_inv is a call that takes them by address
template <class F>
__device__ __forceinline__ F wx_inv(const F& a) {
    typedef typename F::Params P;
    F r = F::one();
    u32 ex[P::N];      // r - 2, word by word: constants once the loops are unrolled
    u64 bw = 2;
    ZK_UNROLL for (int w = 0; w < P::N; ++w) { const u64 t = (u64)P::mod(w) - bw; ex[w] = (u32)t; bw = t >> 63; }
    ZK_UNROLL for (int w = P::N - 1; w >= 0; --w) {
        const u32 e = ex[w];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int b = 31; b >= 0; --b) {
            r = fe_mul(r, r);
            if ((e >> b) & 1) r = fe_mul(r, a);
        }
    }
    return r;
}
// one linear combination of the stream at `pc` over this lane's column of the store: the sum over the RAW terms, empty = 0
// (evaluate_lin, lib.rs:366-372)
template <class F, bool UNI>
__device__ __forceinline__ F wx_lin(const u32* __restrict__ code, u32& pc, const u32* __restrict__ pool, const F* mine, u64 stride) {
    const u32 n = wx_word<UNI>(code[pc]);
    ++pc;
    F acc = F::zero();
    for (u32 t = 0; t < n; ++t) {
        const u32 slot = wx_word<UNI>(code[pc]), ci = wx_word<UNI>(code[pc + 1]);
        pc += 2;
        const F v = wx_load(mine + (u64)slot * stride);
        if (ci == XCOEFF_ONE) {
            acc = fe_add(acc, v);
        } else if (ci == XCOEFF_MINUS_ONE) {
            acc = fe_sub(acc, v);
        } else {
            F c;
            ZK_UNROLL for (int i = 0; i < F::N; ++i) c.v[i] = wx_word<UNI>(pool[(u64)ci * 8 + i]);
            acc = fe_add(acc, fe_mul(v, c));
        }
    }
    return acc;
}
template <class F, bool UNI>
__device__ __forceinline__ F wx_quad(const u32* __restrict__ code, u32& pc, const u32* __restrict__ pool, const F* mine, u64 stride) {      // evaluate_quad, lib.rs:374-378
    const F left = wx_lin<F, UNI>(code, pc, pool, mine, stride);
    const F right = wx_lin<F, UNI>(code, pc, pool, mine, stride);
    return fe_mul(left, right);
}

// ONE instruction of the stream: `op` is its first word and `pc` stands behind it (and behind the instruction afterwards).  The body
// of every opcode, for every kernel of this file: UNI says how a word of the stream is read — the same in every lane (k_exec_program:
// scalar registers), or each lane's own (the level kernels: the lanes of a wave run different instructions).  `i` is the instance,
// `mine` its column of the store.  A failed check leaves its statement in `failed` unless an earlier one is there.  False: `op` is no
// opcode, and nothing was done.
template <class F, bool UNI>
__device__ __forceinline__ bool wx_step(u32 op, const u32* __restrict__ code, u32& pc, const u32* __restrict__ pool, const uint8_t* __restrict__ args, u32 n_args, u32 i,
                                        F* mine, u64 stride, const F& one, u32& failed) {
    switch (op) {
        case XOP_ARG: {
            const u32 k = wx_word<UNI>(code[pc]), slot = wx_word<UNI>(code[pc + 1]);
            pc += 2;
            const F canon = wx_load((const F*)(args + ((u64)i * n_args + k) * 32));
            wx_store(mine + (u64)slot * stride, fe_to_mont(canon));
            return true;
        }
        case XOP_DEFINE: {
            const u32 slot = wx_word<UNI>(code[pc]);
            ++pc;
            const F v = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            wx_store(mine + (u64)slot * stride, v);
            return true;
        }
        case XOP_CHECK: {
            const u32 statement = wx_word<UNI>(code[pc]);
            ++pc;
            const F lhs = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F rhs = wx_lin<F, UNI>(code, pc, pool, mine, stride);
            // `failed` is the caller's own: a plain compare keeps the first it met, and the lane carries on
            failed = (!lhs.equals(rhs) && failed == WX_RAN_THROUGH) ? statement : failed;
            return true;
        }
        case XOP_CONDEQ: {      // [0, 1] for zero, else [1, 1/x]   lib.rs:249-255
            const u32 o0 = wx_word<UNI>(code[pc]), o1 = wx_word<UNI>(code[pc + 1]);
            pc += 2;
            const F x = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const bool z = x.is_zero();
            const F inv = wx_inv(x);      // (every lane inverts: 0 -> 0, then the selection)
            wx_store(mine + (u64)o0 * stride, wx_select(z, F::zero(), one));
            wx_store(mine + (u64)o1 * stride, wx_select(z, one, inv));
            return true;
        }
        case XOP_BITS: {        // out i = bit n - 1 - i of the canonical integer; positions the integer does not have are 0   lib.rs:256-269
            const u32 n = wx_word<UNI>(code[pc]);
            ++pc;
            const F x = fe_from_mont(wx_quad<F, UNI>(code, pc, pool, mine, stride));
            const u32* __restrict__ outs = code + pc;
            pc += n;
            const F zero = F::zero();
            for (u32 k = 0; k + 256 < n; ++k) wx_store(mine + (u64)wx_word<UNI>(outs[k]) * stride, zero);      // positions 256 and above
            ZK_UNROLL for (int w = F::N - 1; w >= 0; --w) {
                const u32 word = x.v[w];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
                for (int b = 31; b >= 0; --b) {
                    const u32 pos = 32u * (u32)w + (u32)b;
                    if (pos < n) wx_store(mine + (u64)wx_word<UNI>(outs[n - 1 - pos]) * stride, wx_select(((word >> b) & 1) != 0, one, zero));
                }
            }
            return true;
        }
        case XOP_DIV: {         // a / b, and 1 for a zero divisor   lib.rs:297
            const u32 o = wx_word<UNI>(code[pc]);
            ++pc;
            const F a = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F b = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F q = fe_mul(a, wx_inv(b));
            wx_store(mine + (u64)o * stride, wx_select(b.is_zero(), one, q));
            return true;
        }
        case XOP_XOR: case XOP_OR: {      // x + y - 2 x y;  x + y - x y   lib.rs:270-281
            const u32 o = wx_word<UNI>(code[pc]);
            ++pc;
            const F x = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F y = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F xy = fe_mul(x, y);
            wx_store(mine + (u64)o * stride, fe_sub(fe_add(x, y), op == XOP_XOR ? fe_dbl(xy) : xy));
            return true;
        }
        case XOP_SHA3: case XOP_SHACH: {
            const u32 o = wx_word<UNI>(code[pc]);
            ++pc;
            const F a = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F b = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            const F c = wx_quad<F, UNI>(code, pc, pool, mine, stride);
            F res;
            if (op == XOP_SHA3) {       // b c - (2 b c - b - c) a   lib.rs:283-288
                const F bc = fe_mul(b, c);
                res = fe_sub(bc, fe_mul(fe_sub(fe_sub(fe_dbl(bc), b), c), a));
            } else {                    // a (b - c) + c   lib.rs:290-295
                res = fe_add(fe_mul(a, fe_sub(b, c)), c);
            }
            wx_store(mine + (u64)o * stride, res);
            return true;
        }
        case XOP_EDIV: {        // the canonical integers: n = q d + r, and q = 0, r = n for d = 0   lib.rs:298-307
            const u32 oq = wx_word<UNI>(code[pc]), orem = wx_word<UNI>(code[pc + 1]);
            pc += 2;
            const F n = fe_from_mont(wx_quad<F, UNI>(code, pc, pool, mine, stride));
            const F d = fe_from_mont(wx_quad<F, UNI>(code, pc, pool, mine, stride));
            // restoring division, a bit at a time from the top: rem < d <= 2^255 before every step, so 2 rem + 1 fits
            F q = F::zero(), rem = F::zero();
            ZK_UNROLL for (int w = F::N - 1; w >= 0; --w) {
                const u32 word = n.v[w];
                u32 qw = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
                for (int b = 31; b >= 0; --b) {
                    u32 carry = (word >> b) & 1;
                    ZK_UNROLL for (int k = 0; k < F::N; ++k) { const u32 nx = rem.v[k] >> 31; rem.v[k] = (rem.v[k] << 1) | carry; carry = nx; }
                    F diff;
                    u64 bw = 0;
                    ZK_UNROLL for (int k = 0; k < F::N; ++k) { const u64 t = (u64)rem.v[k] - d.v[k] - bw; diff.v[k] = (u32)t; bw = t >> 63; }
                    const bool ge = bw == 0;
                    rem = wx_select(ge, diff, rem);
                    qw = (qw << 1) | (ge ? 1u : 0u);
                }
                q.v[w] = qw;
            }
            const bool dz = d.is_zero();
            wx_store(mine + (u64)oq * stride, fe_to_mont(wx_select(dz, F::zero(), q)));
            wx_store(mine + (u64)orem * stride, fe_to_mont(wx_select(dz, n, rem)));
            return true;
        }
        default:
            return false;
    }
}

//   code, pool : the plan's instruction stream and coefficients (xplan.h)
//   args       : count x n_args x 32 B, canonical LE, every one below r (the host has checked)
//   store      : slots x stride elements; work-item i owns element i of every slot
//   verdict    : count words: WX_RAN_THROUGH, or the lowest failing statement
template <class F>
__global__ void __launch_bounds__(WX_BLOCK) k_exec_program(const u32* __restrict__ code, const u32* __restrict__ pool, const uint8_t* __restrict__ args, u32 n_args,
                                                           u32 count, u64 stride, F* store, u32* __restrict__ verdict) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    const u32 i = blockIdx.x * WX_BLOCK + threadIdx.x;
    if (i >= count) return;
    F* mine = store + i;
    const F one = F::one();
    wx_store(mine, one);                      // slot 0: ~one
    u32 failed = WX_RAN_THROUGH;              // (the lane owns its word, and statements come in ascending order: the first met is the lowest)
    u32 pc = 0;
    for (;;) {
        const u32 op = WX_UNIFORM(code[pc]);
        ++pc;
        if (op == XOP_END) break;
        if (!wx_step<F, true>(op, code, pc, pool, args, n_args, i, mine, stride, one, failed)) {
            // (no such word in a stream the compile pass wrote; a lane that met one says so at statement 0 and stops)
            verdict[i] = 0;
            return;
        }
    }
    verdict[i] = failed;
}

// ---- the level-scheduled route (ZKHIP_TUNE_EXEC_WIDE): one work-item per (instruction of a level, instance).  The plan's `sched` holds
// the word offset of every instruction by level (xplan.h: xplan_schedule); the instructions of one level touch no slot another of
// them writes, so they run in no order, and what orders two levels is either the stream (two launches) or, inside k_exec_levels_run,
// the workgroup's barrier.  No launch waits on another workgroup of itself.  The store, the verdict words and the kernels behind
// (gather, file) are those of k_exec_program; a verdict word is the minimum over the instance's failing statements (an ordinary
// atomicMin: "the lowest failing statement" in whatever order the levels met them).

// before the first level: slot 0 (~one) and the verdict word of every instance
template <class F>
__global__ void __launch_bounds__(WX_BLOCK) k_exec_begin(u32 count, F* store, u32* __restrict__ verdict) {
    const u32 i = blockIdx.x * WX_BLOCK + threadIdx.x;
    if (i >= count) return;
    wx_store(store + i, F::one());
    verdict[i] = WX_RAN_THROUGH;
}

// the instruction at word `at` for instance i (a word that is no opcode: verdict 0, as k_exec_program says it)
template <class F>
__device__ __forceinline__ void wx_item(const u32* __restrict__ code, u32 at, const u32* __restrict__ pool, const uint8_t* __restrict__ args, u32 n_args, u32 i,
                                        u64 stride, F* store, u32* verdict) {
    u32 pc = at + 1;
    u32 failed = WX_RAN_THROUGH;
    if (!wx_step<F, false>(code[at], code, pc, pool, args, n_args, i, store + i, stride, F::one(), failed)) failed = 0;
    if (failed != WX_RAN_THROUGH) atomicMin(verdict + i, failed);
}

//   sched      : the plan's schedule; this launch runs its entries [first, first + items): ONE level
// work-item (item along x, instance along y — a grid's y holds 65535, so a workgroup strides over the instances)
template <class F>
__global__ void __launch_bounds__(WX_BLOCK) k_exec_level(const u32* __restrict__ code, const u32* __restrict__ pool, const u32* __restrict__ sched, u32 first, u32 items,
                                                         const uint8_t* __restrict__ args, u32 n_args, u32 count, u64 stride, F* store, u32* verdict) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    const u32 k = blockIdx.x * WX_BLOCK + threadIdx.x;
    if (k >= items) return;
    const u32 at = sched[first + k];
    for (u32 i = blockIdx.y; i < count; i += gridDim.y) wx_item<F>(code, at, pool, args, n_args, i, stride, store, verdict);
}

//   level_start: the plan's; this launch runs levels [lv0, lv1) (counted from 0), each sched[level_start[lv] .. level_start[lv + 1])
// ONE workgroup per instance: it walks a level in strides of its size and meets at a barrier before the next.  The values pass through
// the store in global memory — the barrier orders a workgroup's own stores and loads, which is all a one-workgroup run needs.
static constexpr u32 WX_RUN_BLOCK = 256;      // one wave on every SIMD of a compute unit (the registers of the code object: DESIGN §3)
template <class F>
__global__ void __launch_bounds__(WX_RUN_BLOCK) k_exec_levels_run(const u32* __restrict__ code, const u32* __restrict__ pool, const u32* __restrict__ sched,
                                                                  const u32* __restrict__ level_start, u32 lv0, u32 lv1, const uint8_t* __restrict__ args, u32 n_args,
                                                                  u64 stride, F* store, u32* verdict) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    const u32 i = blockIdx.x;
    for (u32 lv = lv0; lv < lv1; ++lv) {
        const u32 end = level_start[lv + 1];
        for (u32 k = level_start[lv] + threadIdx.x; k < end; k += WX_RUN_BLOCK) wx_item<F>(code, sched[k], pool, args, n_args, i, stride, store, verdict);
        __syncthreads();
    }
}

//   slots      : `count_slots` slot numbers (nullptr: slot j is entry j)
//   verdict    : as k_exec_program left it
//   dst_ptrs   : per instance, where its entries go (nullptr for an instance that gets none) — or, with dst_ptrs == nullptr,
//                dst_flat + i * flat_stride elements, zero-filled for an instance that failed
//   first_one  : entry 0 is written as the constant 1 whatever the slot holds (the z of an assignment)
//   tail       : entries written as 0 behind the last (the two slots of an assignment that receive r and s)
// work-item (instance, entry): the loads of a wave are consecutive, its stores one 32-byte sector each
template <class F>
__global__ void __launch_bounds__(WX_BLOCK) k_exec_gather(const F* __restrict__ store, u64 stride, u32 count, const u32* __restrict__ slots, u64 count_slots,
                                                          const u32* __restrict__ verdict, F* const* __restrict__ dst_ptrs, F* __restrict__ dst_flat, u64 flat_stride,
                                                          int first_one, u32 tail) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    const u32 i = blockIdx.y * WX_BLOCK + threadIdx.x;      // (entries along x: a grid's y holds 65535 at most)
    const u64 j = blockIdx.x;
    if (i >= count || j >= count_slots + tail) return;
    const bool ok = verdict[i] == WX_RAN_THROUGH;
    F* dst = dst_ptrs ? dst_ptrs[i] : dst_flat + (u64)i * flat_stride;
    if (!dst) return;
    F out = F::zero();
    if (ok && j < count_slots) {
        if (first_one && j == 0) out.v[0] = 1;
        else out = fe_from_mont(wx_load(store + (u64)(slots ? slots[j] : (u32)j) * stride + i));
    }
    wx_store(dst + j, out);
}

//   ids, slots : the plan's `entries` witness entries by ascending signed id, and their slots
//   out        : count x file_stride bytes (file_stride a multiple of 8, at least 8 + 40 entries); a failed instance's file is zeros
// work-item (instance, entry; entry 0 also writes the count)
template <class F>
__global__ void __launch_bounds__(WX_BLOCK) k_exec_witness_file(const F* __restrict__ store, u64 stride, u32 count, const long long* __restrict__ ids,
                                                                const u32* __restrict__ slots, u64 entries, const u32* __restrict__ verdict, uint8_t* __restrict__ out,
                                                                u64 file_stride) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    const u32 i = blockIdx.y * WX_BLOCK + threadIdx.x;
    const u64 e = blockIdx.x;
    if (i >= count || e >= entries) return;
    const bool ok = verdict[i] == WX_RAN_THROUGH;
    u64* file = (u64*)(out + (u64)i * file_stride);
    if (e == 0) file[0] = ok ? entries : 0;
    u64* rec = file + 1 + 5 * e;
    F v = F::zero();
    if (ok) v = fe_from_mont(wx_load(store + (u64)slots[e] * stride + i));
    rec[0] = ok ? (u64)ids[e] : 0;
    ZK_UNROLL for (int k = 0; k < 4; ++k) rec[1 + k] = (u64)v.v[2 * k] | (u64)v.v[2 * k + 1] << 32;
}

}  // namespace zk
