//! Hand-written bindings of include/zkhip.h (the subset the adapter needs).  Every function returns 0 on success.
#![allow(non_camel_case_types)]
use std::os::raw::c_char;

#[repr(C)] pub struct zkhip_ctx { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_pk { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_r1cs { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_multi { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_prog { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_assignment { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_queue { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_wplan { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_xplan { _p: [u8; 0] }
#[repr(C)] pub struct zkhip_vk { _p: [u8; 0] }
/// zkhip_queue_submit*: as many proofs in flight as the queue holds; collect one first
pub const ZKHIP_ERR_BUSY: i32 = -6;
/// 16 floats: h2d, matvec, ntt, msm_h, msm_z, finish, total, accum_g1, accum_g2, kernel_ntt, 6 reserved (milliseconds)
#[repr(C)] #[derive(Default, Clone, Copy)] pub struct zkhip_timings { pub ms: [f32; 16] }

pub const ZKHIP_CURVE_BN128: i32 = 0;
pub const ZKHIP_CURVE_BLS12_381: i32 = 1;
pub const ZKHIP_CURVE_BLS12_377: i32 = 2;

pub const ZKHIP_TUNE_PIPE_PLAN: i32 = 28;

extern "C" {
    /// process-wide, before the first context: ask the HIP runtime for `hw_queues` hardware queues (the library never sets
    /// GPU_MAX_HW_QUEUES on its own; 8 for a resident prover, 16 if it is the only context of its process, 0 = leave it)
    pub fn zkhip_init(hw_queues: i32) -> i32;
    pub fn zkhip_ctx_create(device: i32, out: *mut *mut zkhip_ctx) -> i32;
    pub fn zkhip_ctx_free(ctx: *mut zkhip_ctx);
    pub fn zkhip_ctx_tune(ctx: *mut zkhip_ctx, which: i32, value: i32) -> i32;
    pub fn zkhip_last_error(ctx: *const zkhip_ctx) -> *const c_char;
    pub fn zkhip_pk_load_g16(ctx: *mut zkhip_ctx, curve: i32, bytes: *const u8, len: usize, out: *mut *mut zkhip_pk) -> i32;
    pub fn zkhip_pk_load_gm17(ctx: *mut zkhip_ctx, curve: i32, bytes: *const u8, len: usize, out: *mut *mut zkhip_pk) -> i32;
    pub fn zkhip_pk_free(pk: *mut zkhip_pk);
    pub fn zkhip_r1cs_load(ctx: *mut zkhip_ctx, curve: i32, n: u64, l: u64, w: u64,
        rp_a: *const u64, col_a: *const u32, val_a: *const u8,
        rp_b: *const u64, col_b: *const u32, val_b: *const u8,
        rp_c: *const u64, col_c: *const u32, val_c: *const u8, out: *mut *mut zkhip_r1cs) -> i32;
    pub fn zkhip_r1cs_free(cs: *mut zkhip_r1cs);
    pub fn zkhip_prove_g16(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, cs: *const zkhip_r1cs, z: *const u8,
        r: *const u8, s: *const u8, proof_out: *mut u8, timings: *mut zkhip_timings) -> i32;
    pub fn zkhip_prove_gm17(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, cs: *const zkhip_r1cs, z: *const u8,
        d1_d2_r: *const u8, proof_out: *mut u8, timings: *mut zkhip_timings) -> i32;
    // the files the CLI already holds: `out` -> R1CS in ark order, `witness` -> z + inputs (host only, no context)
    pub fn zkhip_prog_parse(bytes: *const u8, len: usize, out: *mut *mut zkhip_prog) -> i32;
    pub fn zkhip_prog_free(prog: *mut zkhip_prog);
    pub fn zkhip_prog_dims(prog: *const zkhip_prog, out: *mut u64 /* [8] */) -> i32;
    pub fn zkhip_prog_r1cs_load(ctx: *mut zkhip_ctx, prog: *const zkhip_prog, out: *mut *mut zkhip_r1cs) -> i32;
    pub fn zkhip_prog_assignment(prog: *const zkhip_prog, witness: *const u8, len: usize, z_out: *mut u8,
        inputs_out: *mut u8, inputs_cap: u64, n_inputs: *mut u64) -> i32;
    // compact assignments: a witness of bits packed on the host (no context), widened on the device into an ordinary resident
    // assignment; `len` of zkhip_assignment_pack >= 32 m says "dense: keep the plain path"
    pub fn zkhip_assignment_pack_bound(m: u64, bytes: *mut u64) -> i32;
    pub fn zkhip_assignment_pack(z: *const u8, m: u64, out: *mut u8, cap: u64, len: *mut u64) -> i32;
    pub fn zkhip_assignment_unpack(packed: *const u8, len: usize, z_out: *mut u8, m_cap: u64, m: *mut u64) -> i32;
    pub fn zkhip_prog_assignment_packed(prog: *const zkhip_prog, witness: *const u8, len: usize, packed_out: *mut u8,
        cap: u64, packed_len: *mut u64, inputs_out: *mut u8, inputs_cap: u64, n_inputs: *mut u64) -> i32;
    pub fn zkhip_assignment_upload_packed(ctx: *mut zkhip_ctx, r1cs: *const zkhip_r1cs, packed: *const u8, len: usize,
        out: *mut *mut zkhip_assignment) -> i32;
    // witness files on the device: a program's column order resident (the plan), and the bytes of a `witness` file tested, ordered
    // and checked there into an ordinary resident assignment — no host pass over the entries; the inputs come back with it
    pub fn zkhip_wplan_create(ctx: *mut zkhip_ctx, prog: *const zkhip_prog, r1cs: *const zkhip_r1cs, out: *mut *mut zkhip_wplan) -> i32;
    pub fn zkhip_wplan_free(plan: *mut zkhip_wplan);
    pub fn zkhip_assignment_upload_witness(ctx: *mut zkhip_ctx, plan: *const zkhip_wplan, witness: *const u8, len: usize,
        inputs_out: *mut u8, inputs_cap: u64, n_inputs: *mut u64, out: *mut *mut zkhip_assignment) -> i32;
    pub fn zkhip_assignment_free(z: *mut zkhip_assignment);
    // witnesses computed on the device: a program's statements compiled once (the plan), then `count` argument lists executed in one
    // launch into resident assignments, the reference's `witness` bytes and the public inputs
    pub fn zkhip_xplan_create(ctx: *mut zkhip_ctx, prog: *const zkhip_prog, r1cs: *const zkhip_r1cs, out_bytes: *const u8, len: usize,
        out: *mut *mut zkhip_xplan) -> i32;
    pub fn zkhip_xplan_free(plan: *mut zkhip_xplan);
    pub fn zkhip_xplan_dims(plan: *const zkhip_xplan, out: *mut u64) -> i32;
    pub fn zkhip_xplan_levels(plan: *const zkhip_xplan, out: *mut u64) -> i32;
    pub fn zkhip_exec_last(ctx: *const zkhip_ctx, out: *mut u64) -> i32;
    pub fn zkhip_compute_witness(ctx: *mut zkhip_ctx, plan: *const zkhip_xplan, count: u32, args: *const u8,
        assignments_out: *mut *mut zkhip_assignment, witness_out: *mut u8, witness_cap_each: u64, inputs_out: *mut u8,
        inputs_cap_each: u64, status: *mut i32, first_statement: *mut u64, first_row: *mut u64) -> i32;
    pub fn zkhip_prove_g16_resident(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, cs: *const zkhip_r1cs, z: *mut zkhip_assignment,
        r: *const u8, s: *const u8, proof_out: *mut u8, timings: *mut zkhip_timings) -> i32;
    // key cache: the resident form of a loaded key as one image
    pub fn zkhip_pk_export_size(pk: *const zkhip_pk, bytes: *mut u64) -> i32;
    pub fn zkhip_pk_export(pk: *const zkhip_pk, out: *mut u8, cap: u64) -> i32;
    pub fn zkhip_pk_import(ctx: *mut zkhip_ctx, bytes: *const u8, len: usize, out: *mut *mut zkhip_pk) -> i32;
    // a resident prover binds its key to its constraint system once (four transforms per proof instead of six, no c)
    pub fn zkhip_pk_bind_r1cs(ctx: *mut zkhip_ctx, pk: *mut zkhip_pk, r1cs: *const zkhip_r1cs) -> i32;
    pub fn zkhip_pk_unbind(pk: *mut zkhip_pk) -> i32;
    pub fn zkhip_pk_is_bound(pk: *const zkhip_pk, r1cs: *const zkhip_r1cs) -> i32;
    // checked proving: Az o Bz == Cz on the device (needs no key), and the context's checked mode for the single-GPU prove calls
    pub fn zkhip_r1cs_check(ctx: *mut zkhip_ctx, r1cs: *const zkhip_r1cs, z: *const u8, z_resident: *mut zkhip_assignment,
        first_row: *mut u64, n_bad: *mut u64) -> i32;
    pub fn zkhip_ctx_set_checked(ctx: *mut zkhip_ctx, on: i32) -> i32;
    pub fn zkhip_ctx_unsatisfied(ctx: *const zkhip_ctx, cap: u32, proof_idx: *mut u32, first_row: *mut u64, n_bad: *mut u64,
        count: *mut u32) -> i32;
    // proof queue: up to ZKHIP_TUNE_SLOTS proofs of one (ctx, pk, r1cs) in flight ACROSS calls — a prover that receives its witnesses one
    // at a time reaches the rate of the batch calls.  While a queue is open its context is pending, as between
    // `split_begin` and `split_end`.  rnd = r | s (64 B, Groth16) or d1 | d2 | r (96 B, GM17); collect is first in, first out
    pub fn zkhip_queue_open(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, r1cs: *const zkhip_r1cs, out: *mut *mut zkhip_queue) -> i32;
    pub fn zkhip_queue_state(q: *const zkhip_queue, capacity: *mut u32, in_flight: *mut u32) -> i32;
    pub fn zkhip_queue_submit(q: *mut zkhip_queue, z: *const u8, z_resident: *mut zkhip_assignment, rnd: *const u8, ticket: *mut u64) -> i32;
    pub fn zkhip_queue_submit_packed(q: *mut zkhip_queue, packed: *const u8, len: usize, rnd: *const u8, ticket: *mut u64) -> i32;
    pub fn zkhip_queue_submit_witness(q: *mut zkhip_queue, plan: *const zkhip_wplan, witness: *const u8, len: usize, rnd: *const u8,
        ticket: *mut u64) -> i32;
    pub fn zkhip_queue_ready(q: *mut zkhip_queue, ready: *mut i32) -> i32;
    pub fn zkhip_queue_collect(q: *mut zkhip_queue, ticket: *mut u64, proof_out: *mut u8, timings: *mut zkhip_timings) -> i32;
    pub fn zkhip_queue_collect_inputs(q: *mut zkhip_queue, ticket: *mut u64, proof_out: *mut u8, inputs_out: *mut u8, inputs_cap: u64,
        n_inputs: *mut u64, timings: *mut zkhip_timings) -> i32;
    pub fn zkhip_queue_close(q: *mut zkhip_queue) -> i32;
    /// a shard of a multi-GPU key (or a whole key, Groth16 or GM17) bound from the key FILE: the transforms need every base once
    pub fn zkhip_pk_bind_r1cs_shard(ctx: *mut zkhip_ctx, pk: *mut zkhip_pk, r1cs: *const zkhip_r1cs, key_bytes: *const u8, len: usize) -> i32;
    // ranks that are separate processes: the witness map of one proof split between two of them.  Between
    // `begin` and `end` the proof is PENDING in its context, which refuses everything but `end`, `abort` and host-only calls
    pub fn zkhip_prove_g16_split_begin(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, r1cs: *const zkhip_r1cs, z: *const u8,
        z_resident: *mut zkhip_assignment, r: *const u8, s: *const u8, half: i32, half_out: *mut u8) -> i32;
    pub fn zkhip_prove_g16_split_end(ctx: *mut zkhip_ctx, pk: *const zkhip_pk, r1cs: *const zkhip_r1cs, other_half: *const u8,
        partial_out: *mut u8, timings: *mut zkhip_timings) -> i32;
    /// the exchange was given up after `begin`: drops the pending proof (ZKHIP_OK also when none is pending)
    pub fn zkhip_prove_g16_split_abort(ctx: *mut zkhip_ctx) -> i32;
    // one proof across several GPUs of this process
    pub fn zkhip_ctx_create_multi(devices: *const i32, n: i32, out: *mut *mut zkhip_multi) -> i32;
    pub fn zkhip_multi_free(m: *mut zkhip_multi);
    pub fn zkhip_multi_last_error(m: *const zkhip_multi) -> *const c_char;
    pub fn zkhip_multi_use_rccl(m: *mut zkhip_multi, on: i32) -> i32;
    pub fn zkhip_multi_exchange(m: *const zkhip_multi) -> *const c_char;
    pub fn zkhip_multi_r1cs_load(m: *mut zkhip_multi, curve: i32, n: u64, l: u64, w: u64,
        rp_a: *const u64, col_a: *const u32, val_a: *const u8,
        rp_b: *const u64, col_b: *const u32, val_b: *const u8,
        rp_c: *const u64, col_c: *const u32, val_c: *const u8) -> i32;
    pub fn zkhip_multi_pk_load_g16(m: *mut zkhip_multi, curve: i32, bytes: *const u8, len: usize) -> i32;
    pub fn zkhip_multi_pk_load_gm17(m: *mut zkhip_multi, curve: i32, bytes: *const u8, len: usize) -> i32;
    /// the members' keys bound to the members' system (one member computes, all install their ranges); bound Groth16 members then
    /// split a proof's witness map between them (zkhip_multi_transform_split, on by default)
    pub fn zkhip_multi_bind(m: *mut zkhip_multi, key_bytes: *const u8, len: usize) -> i32;
    pub fn zkhip_multi_unbind(m: *mut zkhip_multi) -> i32;
    pub fn zkhip_multi_transform_split(m: *mut zkhip_multi, on: i32) -> i32;
    /// the transform domain sharded across the members: stand-alone calls, and the switch for unbound Groth16 proofs (off by default)
    pub fn zkhip_multi_ntt(m: *mut zkhip_multi, curve: i32, log_n: u32, dir: i32, data: *mut u8) -> i32;
    pub fn zkhip_multi_witness_map(m: *mut zkhip_multi, z: *const u8, h_out: *mut u8) -> i32;
    pub fn zkhip_multi_transform_shard(m: *mut zkhip_multi, on: i32) -> i32;
    pub fn zkhip_multi_last_shard(m: *const zkhip_multi) -> i32;
    pub fn zkhip_prove_g16_multi(m: *mut zkhip_multi, z: *const u8, r: *const u8, s: *const u8, proof_out: *mut u8,
        timings: *mut zkhip_timings) -> i32;
    pub fn zkhip_prove_gm17_multi(m: *mut zkhip_multi, z: *const u8, d1_d2_r: *const u8, proof_out: *mut u8,
        timings: *mut zkhip_timings) -> i32;
    // throughput mode: whole key per member, `count` independent proofs dealt over the members
    pub fn zkhip_multi_pk_load_g16_replicas(m: *mut zkhip_multi, curve: i32, bytes: *const u8, len: usize) -> i32;
    pub fn zkhip_prove_g16_multi_batch(m: *mut zkhip_multi, count: u32, z: *const u8, rs: *const u8, proofs_out: *mut u8,
        timings: *mut zkhip_timings) -> i32;
    // verify on the device: one verdict per proof (a verifying key is the head of a proving key; proofs are the records the prove calls write)
    pub fn zkhip_vk_load_g16(ctx: *mut zkhip_ctx, curve: i32, bytes: *const u8, len: usize, out: *mut *mut zkhip_vk) -> i32;
    pub fn zkhip_vk_load_gm17(ctx: *mut zkhip_ctx, curve: i32, bytes: *const u8, len: usize, out: *mut *mut zkhip_vk) -> i32;
    pub fn zkhip_vk_free(vk: *mut zkhip_vk);
    pub fn zkhip_vk_dims(vk: *const zkhip_vk, out: *mut u64) -> i32;
    pub fn zkhip_verify_g16_batch(ctx: *mut zkhip_ctx, vk: *const zkhip_vk, count: u64, proofs: *const u8, inputs: *const u8,
        ok_out: *mut u8) -> i32;
    pub fn zkhip_verify_gm17_batch(ctx: *mut zkhip_ctx, vk: *const zkhip_vk, count: u64, proofs: *const u8, inputs: *const u8,
        ok_out: *mut u8) -> i32;
    pub fn zkhip_pairing_products(ctx: *mut zkhip_ctx, curve: i32, count: u64, pairs_per_item: u32, g1: *const u8, g2: *const u8,
        ok_out: *mut u8) -> i32;
}
