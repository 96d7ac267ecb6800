// wingest.cuh — the device side of witness files (include/zkhip.h "witness files on the device"; the plan's tables and the checks of
// the file's framing are host code: wplan.h).  A ZoKrates `witness` file is fixed-width — u64 count, then count x (i64 id, 32-byte
// canonical LE value) — and the program's column order is known when the program is parsed, so the host reader's pass (test each
// value against r, id -> entry, gather m x 32 B into ark order) is a table lookup and a gather:
//   k_witness_claim   one work-item per ENTRY: value < r, id within the reader's range rule, column of the id, owner[column] =
//                     max(owner, entry + 1) — of the entries that name one id the last in file order wins, as BTreeMap::insert does;
//   k_witness_gather  one work-item per COLUMN: the owner's 32 bytes into z[column]; column 0 is the constant 1 whatever the file
//                     says; a column nobody claimed is missing.
// The verdict is two words next to each other: `flag` (bits below; bit 0 stays k_check_canonical's and k_unpack_assignment's) and
// the lowest missing column.  The host has checked the framing (witness_header_validate) before the bytes are copied: count entries
// are there, and count + 1 fits 32 bits.
#pragma once
#include "devrt.h"
#include "field.cuh"

namespace zk {

static constexpr u32 WIT_FLAG_NON_CANONICAL = 2;      // a value of ANY entry is >= r
static constexpr u32 WIT_FLAG_ID_RANGE = 4;           // an id of ANY entry is outside the reader's range rule
static constexpr u32 WIT_FLAG_MISSING = 8;            // a column has no entry
static constexpr u32 WIT_NO_COLUMN = 0xffffffffu;     // (= WPLAN_NO_COLUMN)
static constexpr u32 WIT_BLOCK = 256;                 // entries per workgroup
static constexpr u32 WIT_RECORD = 40;                 // bytes per entry
// 16-byte slots a workgroup stages: its 256 records start at byte 8 + 10240 b of the file — 8-aligned, never 16-aligned — so the span
// is fetched from the aligned address 8 bytes below and is one slot longer
static constexpr u32 WIT_STAGE_SLOTS = WIT_BLOCK * WIT_RECORD / 16 + 1;

//   raw          : the file as it is, from its byte 0, at a 16-byte aligned device address; `slots` = its 16-byte slots (the buffer
//                  holds that many: the last may end past the file)
//   pos, neg     : the plan's tables (npos, nneg entries): column of id k >= 0 / of id -(k + 1), WIT_NO_COLUMN elsewhere
//   id_bound     : the reader's range rule for this file (witness_id_bound(count))
//   owner        : m words, zero before the launch
template <class F>
__global__ void __launch_bounds__(256) k_witness_claim(const uint4* __restrict__ raw, u64 slots, u64 count, const u32* __restrict__ pos, u64 npos,
                                                       const u32* __restrict__ neg, u64 nneg, u64 id_bound, u32* __restrict__ owner, u32* __restrict__ flag) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    ZK_PRIO_HIGH();
    __shared__ uint4 stage[WIT_STAGE_SLOTS];
    const u32 t = threadIdx.x;
    const u64 blk = blockIdx.x;
    // stage the span: 16-byte loads, consecutive work-items consecutive slots
    const u64 s0 = blk * (WIT_BLOCK * WIT_RECORD / 16);
    const u32 n16 = (u32)(slots - s0 < WIT_STAGE_SLOTS ? slots - s0 : WIT_STAGE_SLOTS);      // (s0 < slots: the workgroup has an entry)
    for (u32 i = t; i < n16; i += WIT_BLOCK) stage[i] = raw[s0 + i];
    __syncthreads();
    const u64 i = blk * WIT_BLOCK + t;
    if (i >= count) return;
    const u32* __restrict__ rec = (const u32*)stage + 2 + 10 * t;      // the record starts 8 bytes into the span: ten words
    u32 bits = 0;
    bool lt = false, decided = false;
    ZK_UNROLL for (int k = F::N - 1; k >= 0; --k) {
        const u32 v = rec[2 + k];
        if (!decided && v != F::Params::mod(k)) { lt = v < F::Params::mod(k); decided = true; }
    }
    if (!lt) bits |= WIT_FLAG_NON_CANONICAL;
    const u64 idw = (u64)rec[1] << 32 | rec[0];
    const bool negative = (idw >> 63) != 0;
    const u64 k = negative ? ~idw : idw;       // -(id + 1) in two's complement
    if (k >= id_bound) {
        bits |= WIT_FLAG_ID_RANGE;
    } else {
        const u32 col = negative ? (k < nneg ? neg[k] : WIT_NO_COLUMN) : (k < npos ? pos[k] : WIT_NO_COLUMN);
        if (col != WIT_NO_COLUMN) atomicMax(&owner[col], (u32)i + 1u);
    }
    if (bits) atomicOr(flag, bits);
}

//   raw        : the file's bytes as above;  owner : as k_witness_claim left it;  z : m x 32 B, canonical integers
//   flag, low  : |= WIT_FLAG_MISSING and min= j for a column j > 0 without an entry (its z[j] is written 0)
template <class F>
__global__ void __launch_bounds__(256) k_witness_gather(const uint8_t* __restrict__ raw, const u32* __restrict__ owner, F* __restrict__ z, u64 m,
                                                        u32* __restrict__ flag, unsigned long long* __restrict__ low) {
    static_assert(F::N == 8, "a scalar field of eight 32-bit words");
    ZK_PRIO_HIGH();
    const u64 j = (u64)blockIdx.x * WIT_BLOCK + threadIdx.x;
    if (j >= m) return;
    uint4* __restrict__ dst = (uint4*)(z + j);
    if (j == 0) {
        dst[0] = make_uint4(1, 0, 0, 0);
        dst[1] = make_uint4(0, 0, 0, 0);
        return;
    }
    const u32 o = owner[j];
    if (o == 0) {
        atomicOr(flag, WIT_FLAG_MISSING);
        atomicMin(low, (unsigned long long)j);
        dst[0] = make_uint4(0, 0, 0, 0);
        dst[1] = make_uint4(0, 0, 0, 0);
        return;
    }
    // the value sits at byte 16 + 40 (o - 1): 8-aligned
    const uint2* __restrict__ src = (const uint2*)(raw + 16 + (u64)WIT_RECORD * (o - 1));
    const uint2 a = src[0], b = src[1], c = src[2], d = src[3];
    dst[0] = make_uint4(a.x, a.y, b.x, b.y);
    dst[1] = make_uint4(c.x, c.y, d.x, d.y);
}

}  // namespace zk
