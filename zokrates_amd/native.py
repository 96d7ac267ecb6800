"""ctypes binding of libzkhip.so — the C ABI declared in include/zkhip.h.

This is plumbing: it adds no arithmetic.  If the HIP library is missing or no GPU is usable, every
entry point raises `ZkhipError`; there is no CPU path behind this module.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# ZKHIP_LIBRARY: development / test hook — load another build of the same C ABI (tests point bench.py at the TEST-ONLY
# emulator build to run its multi-rank plumbing on CPU); unset, the in-tree HIP library is the only candidate
DEFAULT_LIB = os.environ.get("ZKHIP_LIBRARY") or os.path.join(HERE, "libzkhip.so")

CURVE_IDS = {"bn128": 0, "bls12_381": 1, "bls12_377": 2}
FQ_BYTES = {0: 32, 1: 48, 2: 48}

ERR_NAMES = {0: "OK", -1: "BAD_ARG", -2: "PARSE", -3: "NOMEM", -4: "DEVICE", -5: "UNSATISFIED", -6: "BUSY"}


class ZkhipError(RuntimeError):
    """`unsatisfied`: after ZKHIP_ERR_UNSATISFIED from a prove call of a context in checked mode, the (proof index within the call,
    first failing row, failing rows) triples of `zkhip_ctx_unsatisfied`; from `ConstraintSystem.check`, the one triple (0, row, rows).
    `proofs`: what a batch call wrote all the same — the failing proofs' slots zero-filled, the others as without the check."""

    def __init__(self, code, msg):
        super().__init__(f"zkhip error {code} ({ERR_NAMES.get(code, '?')}): {msg}")
        self.code = code
        self.unsatisfied = []
        self.proofs = None


class Timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "h2d_ms", "matvec_ms", "ntt_ms", "msm_h_ms", "msm_z_ms", "finish_ms", "total_ms",
        "kernel_msm_accum_g1_ms", "kernel_msm_accum_g2_ms", "kernel_ntt_ms")] + [("reserved", C.c_float * 6)]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _u8(buf, n=None):
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8)
    if n is not None and a.size != n:
        raise ValueError(f"buffer has {a.size} bytes, expected {n}")
    return a


class Library:
    """One loaded copy of the C ABI."""

    SYMBOLS = [
        "zkhip_device_count", "zkhip_device_pci_bus_id", "zkhip_ctx_create", "zkhip_ctx_free", "zkhip_last_error", "zkhip_pk_load_g16",
        "zkhip_pk_free", "zkhip_pk_dims", "zkhip_r1cs_load", "zkhip_r1cs_free", "zkhip_prove_g16",
        "zkhip_prove_g16_batch", "zkhip_assignment_upload", "zkhip_assignment_free", "zkhip_prove_g16_resident", "zkhip_prove_g16_resident_batch",
        "zkhip_pk_load_g16_shard", "zkhip_partial_size", "zkhip_prove_g16_partial", "zkhip_combine_g16", "zkhip_ntt", "zkhip_witness_map", "zkhip_msm_g1", "zkhip_msm_g2",
        "zkhip_field_op", "zkhip_group_op", "zkhip_setup_g16_size", "zkhip_setup_g16", "zkhip_describe",
        "zkhip_pk_load_gm17", "zkhip_prove_gm17", "zkhip_prove_gm17_resident", "zkhip_prove_gm17_resident_batch",
        "zkhip_setup_gm17_size", "zkhip_setup_gm17", "zkhip_pk_load_gm17_shard", "zkhip_prove_gm17_partial", "zkhip_combine_gm17",
        "zkhip_prog_parse", "zkhip_prog_free", "zkhip_prog_dims", "zkhip_prog_matrix", "zkhip_prog_variable_order",
        "zkhip_prog_r1cs_load", "zkhip_prog_assignment", "zkhip_prog_write_bound", "zkhip_prog_write",
        "zkhip_pk_export_size", "zkhip_pk_export", "zkhip_pk_import",
        "zkhip_pk_bind_r1cs", "zkhip_pk_unbind", "zkhip_pk_is_bound", "zkhip_pk_bind_r1cs_shard", "zkhip_r1cs_fingerprint",
        "zkhip_r1cs_matvec_shape",
        "zkhip_ctx_tune", "zkhip_init", "zkhip_ctx_clock_probe", "zkhip_multi_bind", "zkhip_multi_unbind",
        "zkhip_multi_transform_split", "zkhip_multi_last_split", "zkhip_prove_g16_split_begin", "zkhip_prove_g16_split_end", "zkhip_prove_g16_split_abort",
        "zkhip_ctx_create_multi", "zkhip_multi_free", "zkhip_multi_size", "zkhip_multi_ctx", "zkhip_multi_last_error", "zkhip_multi_r1cs_load",
        "zkhip_multi_pk_load_g16", "zkhip_multi_pk_load_gm17", "zkhip_prove_g16_multi", "zkhip_prove_gm17_multi",
        "zkhip_multi_pk_load_g16_replicas", "zkhip_prove_g16_multi_batch", "zkhip_multi_use_rccl", "zkhip_multi_exchange",
        "zkhip_r1cs_check", "zkhip_ctx_set_checked", "zkhip_ctx_unsatisfied",
        "zkhip_assignment_pack_bound", "zkhip_assignment_pack", "zkhip_assignment_unpack", "zkhip_prog_assignment_packed",
        "zkhip_assignment_upload_packed",
        "zkhip_queue_open", "zkhip_queue_state", "zkhip_queue_submit", "zkhip_queue_submit_packed", "zkhip_queue_ready", "zkhip_queue_collect",
        "zkhip_queue_close",
        "zkhip_multi_ntt", "zkhip_multi_witness_map", "zkhip_multi_transform_shard", "zkhip_multi_last_shard",
        "zkhip_wplan_create", "zkhip_wplan_free", "zkhip_assignment_upload_witness", "zkhip_queue_submit_witness", "zkhip_queue_collect_inputs",
        "zkhip_pairing_products", "zkhip_tower_op", "zkhip_vk_load_g16", "zkhip_vk_load_gm17", "zkhip_vk_free", "zkhip_vk_dims",
        "zkhip_verify_g16_batch", "zkhip_verify_gm17_batch",
        "zkhip_xplan_create", "zkhip_xplan_free", "zkhip_xplan_dims", "zkhip_xplan_levels", "zkhip_exec_last", "zkhip_compute_witness",
    ]

    def __init__(self, path=None):
        self.path = path or DEFAULT_LIB
        if not os.path.exists(self.path):
            raise ZkhipError(-4, f"{self.path} not found: build it with `python -m zokrates_amd.build` "
                                 "(libzkhip has no CPU fallback)")
        L = C.CDLL(self.path)
        vp, u64, u32, i32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_size_t
        pp = C.POINTER(C.c_void_p)
        L.zkhip_device_count.restype = i32
        L.zkhip_device_pci_bus_id.restype = i32; L.zkhip_device_pci_bus_id.argtypes = [i32, C.c_char_p, sz]
        L.zkhip_ctx_create.restype = i32; L.zkhip_ctx_create.argtypes = [i32, pp]
        L.zkhip_ctx_free.restype = None; L.zkhip_ctx_free.argtypes = [vp]
        L.zkhip_ctx_tune.restype = i32; L.zkhip_ctx_tune.argtypes = [vp, i32, i32]
        L.zkhip_ctx_create_multi.restype = i32; L.zkhip_ctx_create_multi.argtypes = [vp, i32, pp]
        L.zkhip_multi_free.restype = None; L.zkhip_multi_free.argtypes = [vp]
        L.zkhip_multi_size.restype = i32; L.zkhip_multi_size.argtypes = [vp]
        L.zkhip_multi_ctx.restype = vp; L.zkhip_multi_ctx.argtypes = [vp, i32]
        L.zkhip_multi_last_error.restype = C.c_char_p; L.zkhip_multi_last_error.argtypes = [vp]
        L.zkhip_multi_use_rccl.restype = i32; L.zkhip_multi_use_rccl.argtypes = [vp, i32]
        L.zkhip_multi_exchange.restype = C.c_char_p; L.zkhip_multi_exchange.argtypes = [vp]
        L.zkhip_multi_r1cs_load.restype = i32; L.zkhip_multi_r1cs_load.argtypes = [vp, i32, u64, u64, u64] + [vp] * 9
        L.zkhip_multi_pk_load_g16.restype = i32; L.zkhip_multi_pk_load_g16.argtypes = [vp, i32, vp, sz]
        L.zkhip_multi_pk_load_gm17.restype = i32; L.zkhip_multi_pk_load_gm17.argtypes = [vp, i32, vp, sz]
        L.zkhip_prove_g16_multi.restype = i32; L.zkhip_prove_g16_multi.argtypes = [vp] * 6
        L.zkhip_prove_gm17_multi.restype = i32; L.zkhip_prove_gm17_multi.argtypes = [vp] * 5
        L.zkhip_multi_pk_load_g16_replicas.restype = i32; L.zkhip_multi_pk_load_g16_replicas.argtypes = [vp, i32, vp, sz]
        L.zkhip_prove_g16_multi_batch.restype = i32; L.zkhip_prove_g16_multi_batch.argtypes = [vp, u32, vp, vp, vp, vp]
        L.zkhip_last_error.restype = C.c_char_p; L.zkhip_last_error.argtypes = [vp]
        L.zkhip_pk_load_g16.restype = i32; L.zkhip_pk_load_g16.argtypes = [vp, i32, vp, sz, pp]
        L.zkhip_pk_free.restype = None; L.zkhip_pk_free.argtypes = [vp]
        L.zkhip_pk_dims.restype = i32; L.zkhip_pk_dims.argtypes = [vp, vp]
        L.zkhip_r1cs_load.restype = i32; L.zkhip_r1cs_load.argtypes = [vp, i32, u64, u64, u64] + [vp] * 9 + [pp]
        L.zkhip_r1cs_free.restype = None; L.zkhip_r1cs_free.argtypes = [vp]
        L.zkhip_prove_g16.restype = i32; L.zkhip_prove_g16.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
        L.zkhip_prove_g16_batch.restype = i32; L.zkhip_prove_g16_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        L.zkhip_assignment_upload.restype = i32; L.zkhip_assignment_upload.argtypes = [vp, vp, vp, pp]
        L.zkhip_assignment_free.restype = None; L.zkhip_assignment_free.argtypes = [vp]
        L.zkhip_prove_g16_resident.restype = i32; L.zkhip_prove_g16_resident.argtypes = [vp] * 8
        L.zkhip_prove_g16_resident_batch.restype = i32; L.zkhip_prove_g16_resident_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        L.zkhip_pk_load_g16_shard.restype = i32; L.zkhip_pk_load_g16_shard.argtypes = [vp, i32, vp, sz, u32, u32, pp]
        L.zkhip_partial_size.restype = i32; L.zkhip_partial_size.argtypes = [i32, vp]
        L.zkhip_prove_g16_partial.restype = i32; L.zkhip_prove_g16_partial.argtypes = [vp] * 9
        L.zkhip_combine_g16.restype = i32; L.zkhip_combine_g16.argtypes = [vp, vp, u32, vp, vp, vp, vp]
        L.zkhip_ntt.restype = i32; L.zkhip_ntt.argtypes = [vp, i32, u32, i32, vp]
        L.zkhip_witness_map.restype = i32; L.zkhip_witness_map.argtypes = [vp, vp, vp, vp]
        L.zkhip_msm_g1.restype = i32; L.zkhip_msm_g1.argtypes = [vp, i32, u64, vp, vp, vp]
        L.zkhip_msm_g2.restype = i32; L.zkhip_msm_g2.argtypes = [vp, i32, u64, vp, vp, vp]
        L.zkhip_field_op.restype = i32; L.zkhip_field_op.argtypes = [vp, i32, i32, i32, u64, vp, vp, vp]
        L.zkhip_group_op.restype = i32; L.zkhip_group_op.argtypes = [vp, i32, i32, i32, i32, u64, vp, vp, vp, vp, vp]
        L.zkhip_pairing_products.restype = i32; L.zkhip_pairing_products.argtypes = [vp, i32, u64, u32, vp, vp, vp]
        L.zkhip_tower_op.restype = i32; L.zkhip_tower_op.argtypes = [vp, i32, i32, u64, vp, vp, vp]
        L.zkhip_vk_load_g16.restype = i32; L.zkhip_vk_load_g16.argtypes = [vp, i32, vp, sz, pp]
        L.zkhip_vk_load_gm17.restype = i32; L.zkhip_vk_load_gm17.argtypes = [vp, i32, vp, sz, pp]
        L.zkhip_vk_free.restype = None; L.zkhip_vk_free.argtypes = [vp]
        L.zkhip_vk_dims.restype = i32; L.zkhip_vk_dims.argtypes = [vp, vp]
        L.zkhip_verify_g16_batch.restype = i32; L.zkhip_verify_g16_batch.argtypes = [vp, vp, u64, vp, vp, vp]
        L.zkhip_verify_gm17_batch.restype = i32; L.zkhip_verify_gm17_batch.argtypes = [vp, vp, u64, vp, vp, vp]
        L.zkhip_setup_g16_size.restype = i32; L.zkhip_setup_g16_size.argtypes = [vp, vp]
        L.zkhip_setup_g16.restype = i32; L.zkhip_setup_g16.argtypes = [vp, vp, vp, vp, vp, vp, u64]
        L.zkhip_describe.restype = i32; L.zkhip_describe.argtypes = [vp, vp, sz]
        L.zkhip_pk_load_gm17.restype = i32; L.zkhip_pk_load_gm17.argtypes = [vp, i32, vp, sz, pp]
        L.zkhip_prove_gm17.restype = i32; L.zkhip_prove_gm17.argtypes = [vp] * 7
        L.zkhip_prove_gm17_resident.restype = i32; L.zkhip_prove_gm17_resident.argtypes = [vp] * 7
        L.zkhip_prove_gm17_resident_batch.restype = i32; L.zkhip_prove_gm17_resident_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        L.zkhip_pk_load_gm17_shard.restype = i32; L.zkhip_pk_load_gm17_shard.argtypes = [vp, i32, vp, sz, u32, u32, pp]
        L.zkhip_prove_gm17_partial.restype = i32; L.zkhip_prove_gm17_partial.argtypes = [vp] * 8
        L.zkhip_combine_gm17.restype = i32; L.zkhip_combine_gm17.argtypes = [vp, vp, u32, vp, vp, vp]
        L.zkhip_setup_gm17_size.restype = i32; L.zkhip_setup_gm17_size.argtypes = [vp, vp]
        L.zkhip_setup_gm17.restype = i32; L.zkhip_setup_gm17.argtypes = [vp, vp, vp, vp, vp, vp, u64]
        L.zkhip_pk_export_size.restype = i32; L.zkhip_pk_export_size.argtypes = [vp, vp]
        L.zkhip_pk_export.restype = i32; L.zkhip_pk_export.argtypes = [vp, vp, u64]
        L.zkhip_pk_import.restype = i32; L.zkhip_pk_import.argtypes = [vp, vp, sz, pp]
        L.zkhip_pk_bind_r1cs.restype = i32; L.zkhip_pk_bind_r1cs.argtypes = [vp, vp, vp]
        L.zkhip_pk_unbind.restype = i32; L.zkhip_pk_unbind.argtypes = [vp]
        L.zkhip_pk_is_bound.restype = i32; L.zkhip_pk_is_bound.argtypes = [vp, vp]
        L.zkhip_pk_bind_r1cs_shard.restype = i32; L.zkhip_pk_bind_r1cs_shard.argtypes = [vp, vp, vp, vp, sz]
        L.zkhip_r1cs_fingerprint.restype = i32; L.zkhip_r1cs_fingerprint.argtypes = [vp, vp, vp]
        L.zkhip_r1cs_matvec_shape.restype = i32; L.zkhip_r1cs_matvec_shape.argtypes = [vp, vp, vp, vp]
        L.zkhip_init.restype = i32; L.zkhip_init.argtypes = [i32]
        L.zkhip_ctx_clock_probe.restype = i32; L.zkhip_ctx_clock_probe.argtypes = [vp, u32, vp]
        L.zkhip_multi_bind.restype = i32; L.zkhip_multi_bind.argtypes = [vp, vp, sz]
        L.zkhip_multi_unbind.restype = i32; L.zkhip_multi_unbind.argtypes = [vp]
        L.zkhip_multi_transform_split.restype = i32; L.zkhip_multi_transform_split.argtypes = [vp, i32]
        L.zkhip_multi_last_split.restype = i32; L.zkhip_multi_last_split.argtypes = [vp]
        L.zkhip_multi_ntt.restype = i32; L.zkhip_multi_ntt.argtypes = [vp, i32, u32, i32, vp]
        L.zkhip_multi_witness_map.restype = i32; L.zkhip_multi_witness_map.argtypes = [vp, vp, vp]
        L.zkhip_multi_transform_shard.restype = i32; L.zkhip_multi_transform_shard.argtypes = [vp, i32]
        L.zkhip_multi_last_shard.restype = i32; L.zkhip_multi_last_shard.argtypes = [vp]
        L.zkhip_prove_g16_split_begin.restype = i32; L.zkhip_prove_g16_split_begin.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.zkhip_prove_g16_split_end.restype = i32; L.zkhip_prove_g16_split_end.argtypes = [vp, vp, vp, vp, vp, vp]
        L.zkhip_prove_g16_split_abort.restype = i32; L.zkhip_prove_g16_split_abort.argtypes = [vp]
        L.zkhip_prog_parse.restype = i32; L.zkhip_prog_parse.argtypes = [vp, sz, pp]
        L.zkhip_prog_free.restype = None; L.zkhip_prog_free.argtypes = [vp]
        L.zkhip_prog_dims.restype = i32; L.zkhip_prog_dims.argtypes = [vp, vp]
        L.zkhip_prog_matrix.restype = i32; L.zkhip_prog_matrix.argtypes = [vp, i32, pp, pp, pp]
        L.zkhip_prog_variable_order.restype = i32; L.zkhip_prog_variable_order.argtypes = [vp, pp]
        L.zkhip_prog_r1cs_load.restype = i32; L.zkhip_prog_r1cs_load.argtypes = [vp, vp, pp]
        L.zkhip_prog_write_bound.restype = i32; L.zkhip_prog_write_bound.argtypes = [u64, u64, u64, vp]
        L.zkhip_prog_write.restype = i32; L.zkhip_prog_write.argtypes = [i32, u64, u64] + [vp] * 9 + [vp, vp, vp, u64, u32, vp, u64, vp]
        L.zkhip_prog_assignment.restype = i32; L.zkhip_prog_assignment.argtypes = [vp, vp, sz, vp, vp, u64, vp]
        L.zkhip_r1cs_check.restype = i32; L.zkhip_r1cs_check.argtypes = [vp] * 6
        L.zkhip_ctx_set_checked.restype = i32; L.zkhip_ctx_set_checked.argtypes = [vp, i32]
        L.zkhip_ctx_unsatisfied.restype = i32; L.zkhip_ctx_unsatisfied.argtypes = [vp, u32, vp, vp, vp, vp]
        L.zkhip_assignment_pack_bound.restype = i32; L.zkhip_assignment_pack_bound.argtypes = [u64, vp]
        L.zkhip_assignment_pack.restype = i32; L.zkhip_assignment_pack.argtypes = [vp, u64, vp, u64, vp]
        L.zkhip_assignment_unpack.restype = i32; L.zkhip_assignment_unpack.argtypes = [vp, sz, vp, u64, vp]
        L.zkhip_prog_assignment_packed.restype = i32; L.zkhip_prog_assignment_packed.argtypes = [vp, vp, sz, vp, u64, vp, vp, u64, vp]
        L.zkhip_assignment_upload_packed.restype = i32; L.zkhip_assignment_upload_packed.argtypes = [vp, vp, vp, sz, pp]
        L.zkhip_queue_open.restype = i32; L.zkhip_queue_open.argtypes = [vp, vp, vp, pp]
        L.zkhip_queue_state.restype = i32; L.zkhip_queue_state.argtypes = [vp, vp, vp]
        L.zkhip_queue_submit.restype = i32; L.zkhip_queue_submit.argtypes = [vp, vp, vp, vp, vp]
        L.zkhip_queue_submit_packed.restype = i32; L.zkhip_queue_submit_packed.argtypes = [vp, vp, sz, vp, vp]
        L.zkhip_queue_ready.restype = i32; L.zkhip_queue_ready.argtypes = [vp, vp]
        L.zkhip_queue_collect.restype = i32; L.zkhip_queue_collect.argtypes = [vp, vp, vp, vp]
        L.zkhip_queue_close.restype = i32; L.zkhip_queue_close.argtypes = [vp]
        L.zkhip_wplan_create.restype = i32; L.zkhip_wplan_create.argtypes = [vp, vp, vp, pp]
        L.zkhip_wplan_free.restype = None; L.zkhip_wplan_free.argtypes = [vp]
        L.zkhip_assignment_upload_witness.restype = i32; L.zkhip_assignment_upload_witness.argtypes = [vp, vp, vp, sz, vp, u64, vp, pp]
        L.zkhip_queue_submit_witness.restype = i32; L.zkhip_queue_submit_witness.argtypes = [vp, vp, vp, sz, vp, vp]
        L.zkhip_queue_collect_inputs.restype = i32; L.zkhip_queue_collect_inputs.argtypes = [vp, vp, vp, vp, u64, vp, vp]
        L.zkhip_xplan_create.restype = i32; L.zkhip_xplan_create.argtypes = [vp, vp, vp, vp, sz, pp]
        L.zkhip_xplan_free.restype = None; L.zkhip_xplan_free.argtypes = [vp]
        L.zkhip_xplan_dims.restype = i32; L.zkhip_xplan_dims.argtypes = [vp, vp]
        L.zkhip_xplan_levels.restype = i32; L.zkhip_xplan_levels.argtypes = [vp, vp]
        L.zkhip_exec_last.restype = i32; L.zkhip_exec_last.argtypes = [vp, vp]
        L.zkhip_compute_witness.restype = i32; L.zkhip_compute_witness.argtypes = [vp, vp, u32, vp, vp, vp, u64, vp, u64, vp, vp, vp]
        self.L = L

    def init(self, hw_queues):
        """`zkhip_init`: the host's explicit request for `hw_queues` HIP hardware queues (GPU_MAX_HW_QUEUES, unless the process set it),
        BEFORE the first HIP call of the process.  The library never touches the environment by itself."""
        rc = self.L.zkhip_init(int(hw_queues))
        if rc != 0:
            raise ZkhipError(rc, self.L.zkhip_last_error(None).decode(errors="replace"))

    def device_count(self):
        return int(self.L.zkhip_device_count())

    def device_pci_bus_id(self, device):
        """"dddd:bb:dd.f" of HIP device `device`: /sys/bus/pci/devices/<that>/numa_node, .../hwmon (None if the runtime cannot tell)."""
        buf = C.create_string_buffer(32)
        if self.L.zkhip_device_pci_bus_id(int(device), buf, 32) != 0:
            return None
        return buf.value.decode().lower() or None


_default = None


def default_library():
    global _default
    if _default is None:
        _default = Library()
    return _default


class Context:
    """`zkhip_ctx`: one GPU, not re-entrant."""

    def __init__(self, device=0, library=None):
        self.lib = library or default_library()
        self.h = C.c_void_p()
        rc = self.lib.L.zkhip_ctx_create(device, C.byref(self.h))
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_last_error(None).decode())

    def _check(self, rc, proofs=None):
        if rc != 0:
            e = ZkhipError(rc, self.lib.L.zkhip_last_error(self.h).decode())
            if rc == -5:
                e.unsatisfied = self.unsatisfied()
                e.proofs = proofs() if proofs else None
            raise e

    def set_checked(self, on=True):
        """`zkhip_ctx_set_checked`: the single-GPU prove calls of this context test Az o Bz == Cz on the device and refuse (ZkhipError
        code -5, `unsatisfied`) an assignment that fails.  None only reports.  Returns the previous setting."""
        was = self.lib.L.zkhip_ctx_set_checked(self.h, -1 if on is None else int(bool(on)))
        if was < 0:       # (refused: a split proof is pending)
            self._check(was)
        return bool(was)

    def unsatisfied(self):
        """`zkhip_ctx_unsatisfied`: [(proof index, first failing row, failing rows)] of the last checked prove call that failed."""
        count = C.c_uint32()
        self.lib.L.zkhip_ctx_unsatisfied(self.h, 0, None, None, None, C.byref(count))
        k = count.value
        idx, row, bad = np.zeros(max(k, 1), dtype=np.uint32), np.zeros(max(k, 1), dtype=np.uint64), np.zeros(max(k, 1), dtype=np.uint64)
        self.lib.L.zkhip_ctx_unsatisfied(self.h, k, _ptr(idx), _ptr(row), _ptr(bad), C.byref(count))
        return [(int(idx[i]), int(row[i]), int(bad[i])) for i in range(k)]

    def describe(self):
        buf = C.create_string_buffer(256)
        self._check(self.lib.L.zkhip_describe(self.h, buf, 256))
        return buf.value.decode()

    TUNABLES = {"msm_c": 1, "msm_waves": 2, "msm_lanes": 3, "msm_min_slice": 4, "fold_scan": 5, "serial": 6, "ntt_single_max_log": 7, "ntt_cols": 8, "slots": 9, "z_gate": 10, "fuse_z": 11, "msm_fused_waves": 12, "stream_jitter": 13, "ntt_max_sublog": 16, "msm_sets": 17, "skip_inf": 18, "b_sort": 19, "heavy_runs": 20, "fold_hg": 25, "ntt_fuse_first": 26, "pipe_plan": 28, "exec_chunk": 29, "alloc_fill": 30, "exec_wide": 31, "exec_wide_min": 32}

    def clock_probe(self, duration_us=2000):
        """`zkhip_ctx_clock_probe`: the shader clock (GHz) the device runs at over the next `duration_us` microseconds — one wavefront
        comparing the cycle counter with the wall clock beside whatever else the device is doing (call it on a SECOND context from a
        second thread while the first proves).  Blocks for the duration."""
        out = C.c_double()
        self._check(self.lib.L.zkhip_ctx_clock_probe(self.h, int(duration_us), C.byref(out)))
        return out.value

    def tune(self, name, value):
        """`zkhip_ctx_tune`: development / measurement knobs (window width, slices, fold form, serial streams ...)."""
        self._check(self.lib.L.zkhip_ctx_tune(self.h, self.TUNABLES[name], int(value)))

    def exec_last(self):
        """`zkhip_exec_last`: (route, chunks, program launches per chunk, wide_min in force) of the last `compute_witness` — route 0
        none yet, 1 one work-item per instance, 2 level-scheduled (`tune("exec_wide", 1)`)."""
        d = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.L.zkhip_exec_last(self.h, _ptr(d)))
        return tuple(int(x) for x in d)

    def upload_witness(self, plan, witness_bytes, want_inputs=True):
        """`zkhip_assignment_upload_witness`: a ZoKrates `witness` file ordered and checked on the device through `plan`
        (`Program.plan`).  Returns (the resident `Assignment`, inputs uint8[k*32] = public_inputs_values), or the assignment alone."""
        wit = _u8(witness_bytes)
        a = Assignment.__new__(Assignment)
        a.ctx = self
        a.h = C.c_void_p()
        cap = plan.n_inputs
        inputs = np.zeros(max(cap, 1) * 32, dtype=np.uint8)
        n_in = C.c_uint64()
        self._check(self.lib.L.zkhip_assignment_upload_witness(self.h, plan.h, _ptr(wit), wit.size, _ptr(inputs) if want_inputs else None, cap,
                                                               C.byref(n_in), C.byref(a.h)))
        return (a, inputs[:32 * n_in.value].copy()) if want_inputs else a

    def compute_witness(self, plan, args, want_files=False, want_inputs=False, want_assignments=True):
        """`zkhip_compute_witness`: the program of `plan` (`Program.exec_plan`) run on the device for a batch.  `args`: count x
        arguments canonical integers (a list of lists of ints, or uint8[count * arguments * 32]).  Returns a `WitnessBatch`: per
        instance `status` (0 or -5), `first_statement`, `first_row` (None where it ran through), the resident `assignments` (None for a
        failed instance), and on request `files` (the reference's `witness` bytes) and `inputs` (public_inputs_values, bytes).  `code`
        is the call's return value (0, or -5 if any instance failed: the others are delivered) and `message` its text."""
        n_args = plan.n_args
        if isinstance(args, np.ndarray) or isinstance(args, (bytes, bytearray)):
            a = _u8(args)
            count = a.size // (32 * n_args) if n_args else 0
        else:
            count = len(args)
            a = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for row in args for v in row), dtype=np.uint8)
        if n_args and a.size != count * n_args * 32:
            raise ValueError(f"arguments have {a.size} bytes, expected {count} x {n_args} x 32")
        handles = (C.c_void_p * max(count, 1))()
        fb, ni = plan.file_bytes, plan.n_inputs
        files = np.zeros(max(count * fb, 1), dtype=np.uint8)
        inputs = np.zeros(max(count * ni * 32, 1), dtype=np.uint8)
        status = np.zeros(max(count, 1), dtype=np.int32)
        st, row = np.zeros(max(count, 1), dtype=np.uint64), np.zeros(max(count, 1), dtype=np.uint64)
        rc = self.lib.L.zkhip_compute_witness(self.h, plan.h, count, _ptr(a) if a.size else None, handles if want_assignments else None,
                                              _ptr(files) if want_files else None, fb, _ptr(inputs) if want_inputs else None, ni, _ptr(status), _ptr(st), _ptr(row))
        if rc not in (0, -5):
            self._check(rc)
        out = WitnessBatch()
        out.code = rc
        out.message = self.lib.L.zkhip_last_error(self.h).decode() if rc else ""
        out.status = [int(x) for x in status[:count]]
        none = (1 << 64) - 1
        out.first_statement = [None if int(x) == none else int(x) for x in st[:count]]
        out.first_row = [None if int(x) == none else int(x) for x in row[:count]]
        out.assignments = []
        for i in range(count):
            if want_assignments and handles[i]:
                z = Assignment.__new__(Assignment)
                z.ctx, z.h = self, C.c_void_p(handles[i])
                out.assignments.append(z)
            else:
                out.assignments.append(None)
        out.files = [files[i * fb:(i + 1) * fb].tobytes() for i in range(count)] if want_files else None
        out.inputs = [inputs[i * ni * 32:(i + 1) * ni * 32].tobytes() for i in range(count)] if want_inputs else None
        return out

    def close(self):
        if self.h:
            self.lib.L.zkhip_ctx_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- primitives ----
    def ntt(self, curve_id, data, direction):
        d = np.array(_u8(data), dtype=np.uint8, copy=True)
        n = d.size // 32
        logn = n.bit_length() - 1
        if n == 0 or (1 << logn) != n:
            raise ValueError("NTT size must be a power of two")
        code = {"fft": 0, "ifft": 1, "coset_fft": 2, "coset_ifft": 3}[direction]
        self._check(self.lib.L.zkhip_ntt(self.h, curve_id, logn, code, _ptr(d)))
        return d

    def msm(self, curve_id, group, bases, scalars):
        nb = FQ_BYTES[curve_id]
        pt = 2 * nb * group
        scalars = _u8(scalars)
        n = scalars.size // 32
        bases = _u8(bases, n * pt)
        out = np.zeros(pt + 1, dtype=np.uint8)
        fn = self.lib.L.zkhip_msm_g1 if group == 1 else self.lib.L.zkhip_msm_g2
        self._check(fn(self.h, curve_id, n, _ptr(bases), _ptr(scalars), _ptr(out)))
        return out.tobytes()

    def field_op(self, curve_id, field, op, a, b):
        nb = 32 if field in (0, 4) else FQ_BYTES[curve_id] * (2 if field in (2, 3) else 1)     # (fields 2, 3: Fq2; 4, 5: unsaturated Fr, Fq — include/zkhip.h)
        a = _u8(a); b = _u8(b, a.size)
        out = np.zeros(a.size, dtype=np.uint8)
        code = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "inv": 4, "mul_call": 5, "sqr_call": 6, "mulsub": 7, "mul_wide": 8, "sqr_wide": 9, "mulsub_wide": 10,
                "sub4": 4, "mul_loose": 5, "sqr_loose": 6, "relax8": 7, "x3_numerator": 11, "bf_sub4": 12, "bf_sub8": 13, "bf_add": 14, "mul_neg_lazy": 15}[op]      # (fields 4, 5)
        self._check(self.lib.L.zkhip_field_op(self.h, curve_id, field, code, a.size // nb, _ptr(a), _ptr(b), _ptr(out)))
        return out

    GROUP_OPS = ["madd_acc", "madd_cold", "madd_hot", "add_acc", "add_from", "add", "add_to", "dbl", "dbl_inl", "dbl_acc", "dbl_affine", "dbl_affine_hot",
                 "neg_u", "to_affine", "to_affine_u", "mul_words", "mul_u32", "mul_small", "madd_acc_neg", "add_from_neg"]       # (the ids of include/zkhip.h, in order)

    def group_op(self, curve_id, group, form, op, a, b, k, flags):
        """TESTS ONLY (zkhip_group_op): a, b: uint32 arrays of count x 4 coordinates of raw limbs, k: count x 8 words, flags: count
        bytes; returns the raw result limbs in the shape of `a`."""
        a = np.ascontiguousarray(a, dtype=np.uint32); b = np.ascontiguousarray(b, dtype=np.uint32)
        k = np.ascontiguousarray(k, dtype=np.uint32); flags = np.ascontiguousarray(flags, dtype=np.uint8)
        count = flags.size
        if a.shape != b.shape or a.size % max(count, 1) or k.size != 8 * count:
            raise ValueError("operand shapes")
        out = np.zeros_like(a)
        self._check(self.lib.L.zkhip_group_op(self.h, curve_id, group, form, self.GROUP_OPS.index(op) if isinstance(op, str) else op, count,
                                              _ptr(a), _ptr(b), _ptr(k), _ptr(flags), _ptr(out)))
        return out

    def pairing_products(self, curve_id, pairs_per_item, g1, g2):
        """zkhip_pairing_products: g1 / g2 are the point records of a proof (canonical little-endian coordinates and a flag byte, non-zero =
        the point at infinity), count x pairs_per_item of each; returns count bytes, 1 where the product of the item's pairings is 1.
        `ok` starts as 0xff so that a caller can see a call that wrote nothing."""
        fq = FQ_BYTES[curve_id]
        g1 = _u8(g1); g2 = _u8(g2)
        n = g1.size // (2 * fq + 1)
        if pairs_per_item < 1 or g1.size != n * (2 * fq + 1) or g2.size != n * (4 * fq + 1) or n % pairs_per_item:
            raise ValueError("operand shapes")
        ok = np.full(n // pairs_per_item, 0xff, dtype=np.uint8)
        self.last_ok = ok
        self._check(self.lib.L.zkhip_pairing_products(self.h, curve_id, n // pairs_per_item, pairs_per_item, _ptr(g1), _ptr(g2), _ptr(ok)))
        return ok

    last_ok = None      # the verdict buffer of the last pairing_products / verify_*_batch call, also where the call failed (tests: 0xff = not written)
    TOWER_OPS = ["mul", "sqr", "mul_line", "inv", "frobenius", "conj6"]       # (the ids of include/zkhip.h, in order)

    def tower_op(self, curve_id, op, a, b):
        """TESTS ONLY (zkhip_tower_op): a, b: uint32 arrays of count x 6 x 2 x N raw limbs; returns the raw result limbs in the shape of `a`."""
        a = np.ascontiguousarray(a, dtype=np.uint32); b = np.ascontiguousarray(b, dtype=np.uint32)
        if a.shape != b.shape or a.ndim != 4 or a.shape[1:3] != (6, 2):
            raise ValueError("operand shapes")
        out = np.zeros_like(a)
        self._check(self.lib.L.zkhip_tower_op(self.h, curve_id, self.TOWER_OPS.index(op) if isinstance(op, str) else op, a.shape[0], _ptr(a), _ptr(b), _ptr(out)))
        return out


class ProvingKey:
    """`zkhip_pk`: an ark `proving.key` resident on the GPU in MSM-ready layout."""

    def __init__(self, ctx, curve_id, data, rank=0, world=1, scheme="g16"):
        """world > 1: load only rank's share of the bases (one proof sharded over several GPUs).
        scheme = "gm17": an ark-gm17 proving key (zkhip_pk_load_gm17; m = SAP variables, hlen = len(g_gamma2_z_t))."""
        self.ctx = ctx
        self.curve_id = curve_id
        self.rank, self.world = rank, world
        self.scheme = scheme
        data = _u8(data)
        self.h = C.c_void_p()
        if scheme == "gm17" and world == 1:
            ctx._check(ctx.lib.L.zkhip_pk_load_gm17(ctx.h, curve_id, _ptr(data), data.size, C.byref(self.h)))
        elif scheme == "gm17":
            ctx._check(ctx.lib.L.zkhip_pk_load_gm17_shard(ctx.h, curve_id, _ptr(data), data.size, rank, world, C.byref(self.h)))
        elif world == 1:
            ctx._check(ctx.lib.L.zkhip_pk_load_g16(ctx.h, curve_id, _ptr(data), data.size, C.byref(self.h)))
        else:
            ctx._check(ctx.lib.L.zkhip_pk_load_g16_shard(ctx.h, curve_id, _ptr(data), data.size, rank, world, C.byref(self.h)))
        self._dims()

    def _dims(self):
        d = np.zeros(4, dtype=np.uint64)
        self.ctx._check(self.ctx.lib.L.zkhip_pk_dims(self.h, _ptr(d)))
        self.m, self.hlen, self.w, self.l = (int(x) for x in d)

    def export_image(self):
        """The resident (device-layout) form of this key as bytes (`zkhip_pk_export`): what a key cache stores — level 0 of the
        five base tables; the import recomputes the window multiples on the device."""
        size = C.c_uint64()
        self.ctx._check(self.ctx.lib.L.zkhip_pk_export_size(self.h, C.byref(size)))
        out = np.zeros(size.value, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.L.zkhip_pk_export(self.h, _ptr(out), size.value))
        return out

    @classmethod
    def from_image(cls, ctx, curve_id, image, scheme="g16"):
        """`zkhip_pk_import`: no parsing, no conversion — five host-to-device copies."""
        self = cls.__new__(cls)
        self.ctx, self.curve_id, self.rank, self.world, self.scheme = ctx, curve_id, 0, 1, scheme
        image = _u8(image)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_pk_import(ctx.h, _ptr(image), image.size, C.byref(self.h)))
        self._dims()
        return self

    def bind(self, cs):
        """`zkhip_pk_bind_r1cs`: apply the quotient's transforms to this key's bases once, for the constraint system `cs` — proofs
        over (this key, cs) then take four transforms instead of six and skip c; the proof bytes do not change."""
        self.ctx._check(self.ctx.lib.L.zkhip_pk_bind_r1cs(self.ctx.h, self.h, cs.h))

    def bind_shard(self, cs, key_bytes):
        """`zkhip_pk_bind_r1cs_shard`: the same for a SHARD (or a whole key) from the key file — the transforms need every base of
        the key once; this key keeps its index ranges of the bound tables."""
        data = _u8(key_bytes)
        self.ctx._check(self.ctx.lib.L.zkhip_pk_bind_r1cs_shard(self.ctx.h, self.h, cs.h, _ptr(data), data.size))

    def unbind(self):
        self.ctx._check(self.ctx.lib.L.zkhip_pk_unbind(self.h))

    def is_bound(self, cs):
        return bool(self.ctx.lib.L.zkhip_pk_is_bound(self.h, cs.h))

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_pk_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VerificationKey:
    """`zkhip_vk`: ark's VerifyingKey (the head of a `proving.key`, so the whole key's bytes serve), admitted and resident on the GPU."""

    def __init__(self, ctx, curve_id, data, scheme="g16"):
        self.ctx, self.curve_id, self.scheme = ctx, curve_id, scheme
        data = _u8(data)
        self.h = C.c_void_p()
        load = ctx.lib.L.zkhip_vk_load_gm17 if scheme == "gm17" else ctx.lib.L.zkhip_vk_load_g16
        ctx._check(load(ctx.h, curve_id, _ptr(data), data.size, C.byref(self.h)))
        d = np.zeros(2, dtype=np.uint64)
        ctx._check(ctx.lib.L.zkhip_vk_dims(self.h, _ptr(d)))
        self.l = int(d[0])

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_vk_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _verify_batch(fn, ctx, vk, proofs, inputs):
    nb = FQ_BYTES[vk.curve_id]
    proofs = _u8(b"".join(proofs) if isinstance(proofs, (list, tuple)) else proofs)
    count = proofs.size // (8 * nb + 3)
    inputs = _u8(inputs, count * vk.l * 32)
    if proofs.size != count * (8 * nb + 3):
        raise ValueError("proof records")
    ok = np.full(count, 0xff, dtype=np.uint8)
    ctx.last_ok = ok
    ctx._check(fn(ctx.h, vk.h, count, _ptr(proofs), _ptr(inputs) if inputs.size else None, _ptr(ok)))
    return ok


def verify_g16_batch(ctx, vk, proofs, inputs):
    """`zkhip_verify_g16_batch`: proofs = the records zkhip_prove_g16 writes (bytes or a list of them), inputs = count x l x 32 B
    canonical little-endian; returns count bytes of 0 / 1 (the buffer starts as 0xff: a failed call leaves it so)."""
    return _verify_batch(ctx.lib.L.zkhip_verify_g16_batch, ctx, vk, proofs, inputs)


def verify_gm17_batch(ctx, vk, proofs, inputs):
    """`zkhip_verify_gm17_batch`: as verify_g16_batch for GM17 proofs and keys."""
    return _verify_batch(ctx.lib.L.zkhip_verify_gm17_batch, ctx, vk, proofs, inputs)


class ConstraintSystem:
    """`zkhip_r1cs`: CSR matrices in ark variable order, resident on the GPU."""

    def __init__(self, ctx, curve_id, n, l, w, mats):
        self.ctx = ctx
        self.curve_id = curve_id
        self.n, self.l, self.w = n, l, w
        self.m = l + w
        args, keep = [], []
        for rp, col, val in mats:
            rp = np.ascontiguousarray(rp, dtype=np.uint64)
            col = np.ascontiguousarray(col, dtype=np.uint32)
            val = _u8(val)
            if rp.size != n + 1 or val.size != col.size * 32:
                raise ValueError("CSR shape mismatch")
            keep += [rp, col, val]
            args += [_ptr(rp), _ptr(col), _ptr(val)]
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_r1cs_load(ctx.h, curve_id, n, l, w, *args, C.byref(self.h)))

    def fingerprint(self):
        """`zkhip_r1cs_fingerprint`: the checksum a key image remembers of the system its bound tables were made for."""
        out = np.zeros(2, dtype=np.uint64)
        self.ctx._check(self.ctx.lib.L.zkhip_r1cs_fingerprint(self.ctx.h, self.h, _ptr(out)))
        return int(out[0]), int(out[1])

    def matvec_shape(self):
        """`zkhip_r1cs_matvec_shape`: ((lanes per row of A, B, C), rows left to k_matvec_long, rows left to k_matvec_huge) as a
        proof over this system launches its mat-vec."""
        lanes = np.zeros(3, dtype=np.int32)
        n_long, n_huge = C.c_uint64(), C.c_uint64()
        rc = self.ctx.lib.L.zkhip_r1cs_matvec_shape(self.h, _ptr(lanes), C.byref(n_long), C.byref(n_huge))
        if rc != 0:
            raise ZkhipError(rc, "zkhip_r1cs_matvec_shape")
        return tuple(int(g) for g in lanes), int(n_long.value), int(n_huge.value)

    def check(self, z):
        """`zkhip_r1cs_check`: Az o Bz == Cz on the device for a host assignment (uint8[m*32]) or a resident `Assignment`.
        Returns (first failing row or None, failing rows); never raises for an unsatisfied system."""
        first, bad = C.c_uint64(), C.c_uint64()
        if isinstance(z, Assignment):
            zp, za = None, z.h
        else:
            z = _u8(z, self.m * 32)
            zp, za = _ptr(z), None
        rc = self.ctx.lib.L.zkhip_r1cs_check(self.ctx.h, self.h, zp, za, C.byref(first), C.byref(bad))
        if rc not in (0, -5):
            self.ctx._check(rc)
        return (None if rc == 0 else int(first.value)), int(bad.value)

    def witness_map(self, z):
        N = 1
        while N < self.n + self.l:
            N *= 2
        z = _u8(z, self.m * 32)
        out = np.zeros(N * 32, dtype=np.uint8)
        self.ctx._check(self.ctx.lib.L.zkhip_witness_map(self.ctx.h, self.h, _ptr(z), _ptr(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_r1cs_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Assignment:
    """`zkhip_assignment`: a full assignment z (m x 32 B canonical LE, z[0] = 1) resident in HBM."""

    def __init__(self, ctx, cs, z):
        self.ctx = ctx
        z = _u8(z, cs.m * 32)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_assignment_upload(ctx.h, cs.h, _ptr(z), C.byref(self.h)))

    @classmethod
    def from_packed(cls, ctx, cs, packed):
        """`zkhip_assignment_upload_packed`: the same resident assignment from its packed form (`pack_assignment`,
        `Program.assignment_packed`), widened on the device."""
        self = cls.__new__(cls)
        self.ctx = ctx
        packed = _u8(packed)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_assignment_upload_packed(ctx.h, cs.h, _ptr(packed), packed.size, C.byref(self.h)))
        return self

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_assignment_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_bound(m, library=None):
    """`zkhip_assignment_pack_bound`: the length of a packing of m elements that are all 32 bytes wide."""
    lib = library or default_library()
    out = C.c_uint64()
    rc = lib.L.zkhip_assignment_pack_bound(int(m), C.byref(out))
    if rc != 0:
        raise ZkhipError(rc, lib.L.zkhip_last_error(None).decode())
    return int(out.value)


def pack_assignment(z, library=None, cap=None):
    """`zkhip_assignment_pack` (host only): uint8[m*32] -> the packed form as uint8[len].  len >= 32 m says the witness is dense
    and the plain upload is the one to use.  `cap`: the size of the output buffer (default: the bound)."""
    lib = library or default_library()
    z = _u8(z)
    if z.size % 32:
        raise ValueError("an assignment is m x 32 bytes")
    m = z.size // 32
    cap = pack_bound(m, lib) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_uint64()
    rc = lib.L.zkhip_assignment_pack(_ptr(z), m, _ptr(out), cap, C.byref(n))
    if rc != 0:
        raise ZkhipError(rc, lib.L.zkhip_last_error(None).decode())
    return out[:n.value].copy()


def unpack_assignment(packed, library=None, m_cap=None):
    """`zkhip_assignment_unpack` (host only): the packed form -> uint8[m*32].  `m_cap`: the elements the output may hold
    (default: the count the header names, within what a buffer of that length can hold)."""
    lib = library or default_library()
    packed = _u8(packed)
    if m_cap is None:
        m_cap = min(int.from_bytes(packed[8:16].tobytes(), "little"), 4 * packed.size) if packed.size >= 16 else 0
    z = np.zeros(max(int(m_cap), 1) * 32, dtype=np.uint8)
    m = C.c_uint64()
    rc = lib.L.zkhip_assignment_unpack(_ptr(packed), packed.size, _ptr(z), int(m_cap), C.byref(m))
    if rc != 0:
        raise ZkhipError(rc, lib.L.zkhip_last_error(None).decode())
    return z[:32 * m.value].copy()


def prove_g16_resident(ctx, pk, cs, assignment, r, s, want_timings=False):
    """Like prove_g16 with the assignment already on the GPU."""
    nb = FQ_BYTES[pk.curve_id]
    rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
    sb = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    out = np.zeros(8 * nb + 3, dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_g16_resident(ctx.h, pk.h, cs.h, assignment.h, _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm)))
    return (out.tobytes(), tm.as_dict()) if want_timings else out.tobytes()


def prove_g16_split_begin(ctx, pk_shard, cs, z, r, s, half):
    """`zkhip_prove_g16_split_begin`: this rank's half (0: a, 1: b on the coset) of a split witness map, as uint8[N * 32]; the proof
    stays in flight until prove_g16_split_end."""
    n_dom = pk_shard.hlen + 1
    out = np.zeros(n_dom * 32, dtype=np.uint8)
    rb, sb = int(r).to_bytes(32, "little"), int(s).to_bytes(32, "little")
    if isinstance(z, Assignment):
        zp, za = None, z.h
    else:
        zp, za = _ptr(_u8(z, cs.m * 32)), None
    ctx._check(ctx.lib.L.zkhip_prove_g16_split_begin(ctx.h, pk_shard.h, cs.h, zp, za, rb, sb, int(half), _ptr(out)))
    return out


def prove_g16_split_end(ctx, pk_shard, cs, other_half):
    """`zkhip_prove_g16_split_end`: the partner's half in, this rank's partial record out."""
    other = _u8(other_half, (pk_shard.hlen + 1) * 32)
    out = np.zeros(partial_size(ctx, pk_shard.curve_id), dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_g16_split_end(ctx.h, pk_shard.h, cs.h, _ptr(other), _ptr(out), C.byref(tm)))
    return out


def prove_g16_split_abort(ctx):
    """`zkhip_prove_g16_split_abort`: drop the split proof pending in `ctx` (the exchange was given up); nothing pending: no-op."""
    ctx._check(ctx.lib.L.zkhip_prove_g16_split_abort(ctx.h))


def partial_size(ctx, curve_id):
    n = C.c_uint64()
    ctx._check(ctx.lib.L.zkhip_partial_size(curve_id, C.byref(n)))
    return int(n.value)


def prove_g16_partial(ctx, pk_shard, cs, z, r, s, want_timings=False):
    """One rank's share of a proof: z is a host assignment (uint8[m*32]) or an `Assignment`.  Returns the partial record."""
    rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
    sb = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    out = np.zeros(partial_size(ctx, pk_shard.curve_id), dtype=np.uint8)
    tm = Timings()
    if isinstance(z, Assignment):
        zp, za = None, z.h
    else:
        z = _u8(z, cs.m * 32)
        zp, za = _ptr(z), None
    ctx._check(ctx.lib.L.zkhip_prove_g16_partial(ctx.h, pk_shard.h, cs.h, zp, za, _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm)))
    return (out, tm.as_dict()) if want_timings else out


def combine_g16(ctx, pk, partials, r, s):
    """Adds the ranks' partial records (list of uint8 arrays) and assembles the proof."""
    nb = FQ_BYTES[pk.curve_id]
    buf = np.ascontiguousarray(np.concatenate([_u8(p) for p in partials]))
    rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
    sb = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    out = np.zeros(8 * nb + 3, dtype=np.uint8)
    ctx._check(ctx.lib.L.zkhip_combine_g16(ctx.h, pk.h, len(partials), _ptr(buf), _ptr(rb), _ptr(sb), _ptr(out)))
    return out.tobytes()


def setup_g16(ctx, cs, toxic, g1=None, g2=None):
    """Groth16 setup on the GPU: `toxic` = (alpha, beta, gamma, delta, tau) ints; returns the ark-format proving key bytes."""
    size = C.c_uint64()
    ctx._check(ctx.lib.L.zkhip_setup_g16_size(cs.h, C.byref(size)))
    tb = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in toxic), dtype=np.uint8)
    out = np.zeros(size.value, dtype=np.uint8)
    g1p = _ptr(_u8(g1)) if g1 is not None else None
    g2p = _ptr(_u8(g2)) if g2 is not None else None
    ctx._check(ctx.lib.L.zkhip_setup_g16(ctx.h, cs.h, _ptr(tb), g1p, g2p, _ptr(out), size.value))
    return out


def prove_g16(ctx, pk, cs, z, r, s, want_timings=False):
    """Raw proof bytes (8*sz(Fq)+3) for assignment z (m*32 B canonical LE) and blinding scalars r, s (ints)."""
    nb = FQ_BYTES[pk.curve_id]
    z = _u8(z, cs.m * 32)
    rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
    sb = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
    out = np.zeros(8 * nb + 3, dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_g16(ctx.h, pk.h, cs.h, _ptr(z), _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm)))
    return (out.tobytes(), tm.as_dict()) if want_timings else out.tobytes()


def _split_proofs(out, count, step):
    return [out[i * step:(i + 1) * step].tobytes() for i in range(count)]


def prove_g16_resident_batch(ctx, pk, cs, assignments, rs):
    """Pipelined proofs over resident assignments (may repeat); rs: list of (r, s) ints.  Returns (proofs, timings)."""
    nb = FQ_BYTES[pk.curve_id]
    count = len(rs)
    assert len(assignments) == count
    handles = (C.c_void_p * count)(*[a.h for a in assignments])
    rsb = np.frombuffer(b"".join(int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little") for r, s in rs), dtype=np.uint8)
    out = np.zeros(count * (8 * nb + 3), dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_g16_resident_batch(ctx.h, pk.h, cs.h, count, handles, _ptr(rsb), _ptr(out), C.byref(tm)), lambda: _split_proofs(out, count, 8 * nb + 3))
    return _split_proofs(out, count, 8 * nb + 3), tm.as_dict()


def prove_g16_batch(ctx, pk, cs, zs, rs):
    """zs: uint8[count*m*32]; rs: list of (r, s) ints.  Returns (list of raw proofs, summed timings)."""
    nb = FQ_BYTES[pk.curve_id]
    count = len(rs)
    zs = _u8(zs, count * pk.m * 32)
    rsb = np.frombuffer(b"".join(int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little") for r, s in rs), dtype=np.uint8)
    out = np.zeros(count * (8 * nb + 3), dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_g16_batch(ctx.h, pk.h, cs.h, count, _ptr(zs), _ptr(rsb), _ptr(out), C.byref(tm)), lambda: _split_proofs(out, count, 8 * nb + 3))
    return _split_proofs(out, count, 8 * nb + 3), tm.as_dict()


# ---- GM17 (BASELINE.json config 5) ----
def _rnd96(d1, d2, r):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in (d1, d2, r)), dtype=np.uint8)


def setup_gm17(ctx, cs, toxic, g1=None, g2=None):
    """GM17 setup on the GPU: `toxic` = (alpha, beta, gamma, t) ints; returns the ark-gm17-format proving key bytes."""
    size = C.c_uint64()
    ctx._check(ctx.lib.L.zkhip_setup_gm17_size(cs.h, C.byref(size)))
    tb = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in toxic), dtype=np.uint8)
    out = np.zeros(size.value, dtype=np.uint8)
    g1p = _ptr(_u8(g1)) if g1 is not None else None
    g2p = _ptr(_u8(g2)) if g2 is not None else None
    ctx._check(ctx.lib.L.zkhip_setup_gm17(ctx.h, cs.h, _ptr(tb), g1p, g2p, _ptr(out), size.value))
    return out


def prove_gm17(ctx, pk, cs, z, d1, d2, r, want_timings=False):
    """Raw proof bytes (8*sz(Fq)+3) for assignment z (host bytes or a resident `Assignment`) and blinding scalars d1, d2, r."""
    nb = FQ_BYTES[pk.curve_id]
    rnd = _rnd96(d1, d2, r)
    out = np.zeros(8 * nb + 3, dtype=np.uint8)
    tm = Timings()
    if isinstance(z, Assignment):
        ctx._check(ctx.lib.L.zkhip_prove_gm17_resident(ctx.h, pk.h, cs.h, z.h, _ptr(rnd), _ptr(out), C.byref(tm)))
    else:
        z = _u8(z, cs.m * 32)
        ctx._check(ctx.lib.L.zkhip_prove_gm17(ctx.h, pk.h, cs.h, _ptr(z), _ptr(rnd), _ptr(out), C.byref(tm)))
    return (out.tobytes(), tm.as_dict()) if want_timings else out.tobytes()


def prove_gm17_partial(ctx, pk_shard, cs, z, d1, d2, r):
    """One rank's share of a GM17 proof: z is a host assignment or an `Assignment`.  Returns the partial record."""
    rnd = _rnd96(d1, d2, r)
    out = np.zeros(partial_size(ctx, pk_shard.curve_id), dtype=np.uint8)
    tm = Timings()
    if isinstance(z, Assignment):
        zp, za = None, z.h
    else:
        z = _u8(z, cs.m * 32)
        zp, za = _ptr(z), None
    ctx._check(ctx.lib.L.zkhip_prove_gm17_partial(ctx.h, pk_shard.h, cs.h, zp, za, _ptr(rnd), _ptr(out), C.byref(tm)))
    return out


def combine_gm17(ctx, pk, partials, d1, d2, r):
    nb = FQ_BYTES[pk.curve_id]
    buf = np.ascontiguousarray(np.concatenate([_u8(p) for p in partials]))
    rnd = _rnd96(d1, d2, r)
    out = np.zeros(8 * nb + 3, dtype=np.uint8)
    ctx._check(ctx.lib.L.zkhip_combine_gm17(ctx.h, pk.h, len(partials), _ptr(buf), _ptr(rnd), _ptr(out)))
    return out.tobytes()


def prove_gm17_resident_batch(ctx, pk, cs, assignments, rnds):
    """Pipelined GM17 proofs over resident assignments (may repeat); rnds: list of (d1, d2, r) ints."""
    nb = FQ_BYTES[pk.curve_id]
    count = len(rnds)
    assert len(assignments) == count
    handles = (C.c_void_p * count)(*[a.h for a in assignments])
    rb = np.ascontiguousarray(np.concatenate([_rnd96(*t) for t in rnds])) if count else np.zeros(1, dtype=np.uint8)
    out = np.zeros(max(count, 1) * (8 * nb + 3), dtype=np.uint8)
    tm = Timings()
    ctx._check(ctx.lib.L.zkhip_prove_gm17_resident_batch(ctx.h, pk.h, cs.h, count, handles, _ptr(rb), _ptr(out), C.byref(tm)), lambda: _split_proofs(out, count, 8 * nb + 3))
    return _split_proofs(out, count, 8 * nb + 3), tm.as_dict()


# ---- the proof queue: proofs in flight across calls ----
BUSY = -6


class ProofQueue:
    """`zkhip_queue`: up to `capacity` proofs of one (context, key, constraint system) in flight ACROSS calls — the pipeline of the
    batch calls with the caller as the loop.  `submit` / `submit_packed` return the ticket, `collect` the oldest proof (FIFO); a
    submit at capacity raises ZkhipError with code BUSY (-6).  While it is open its context refuses every other proving call
    (include/zkhip.h, Conventions); use it as a context manager or `close` it."""

    def __init__(self, ctx, pk, cs):
        self.ctx, self.pk, self.cs = ctx, pk, cs
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_queue_open(ctx.h, pk.h, cs.h, C.byref(self.h)))
        self.proof_bytes = 8 * FQ_BYTES[pk.curve_id] + 3
        self.rnd_bytes = 96 if pk.scheme == "gm17" else 64

    def _rnd(self, rnd):
        """(r, s) / (d1, d2, r) as ints, or the 64 / 96 bytes themselves (a numpy array is passed as it is, not copied)"""
        if isinstance(rnd, (tuple, list)):
            rnd = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in rnd), dtype=np.uint8)
        return _u8(rnd, self.rnd_bytes)

    def state(self):
        """`zkhip_queue_state`: (capacity, proofs in flight)"""
        cap, n = C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.lib.L.zkhip_queue_state(self.h, C.byref(cap), C.byref(n)))
        return int(cap.value), int(n.value)

    def submit(self, z, rnd):
        """`zkhip_queue_submit`: z is a host assignment (uint8[m*32]) or a resident `Assignment`, which must stay alive until its
        ticket is collected; the host buffers are the caller's again when this returns.  Returns the ticket."""
        rb = self._rnd(rnd)
        ticket = C.c_uint64()
        if isinstance(z, Assignment):
            zp, za = None, z.h
        else:
            z = _u8(z, self.cs.m * 32)
            zp, za = _ptr(z), None
        self.ctx._check(self.ctx.lib.L.zkhip_queue_submit(self.h, zp, za, _ptr(rb), C.byref(ticket)))
        return int(ticket.value)

    def submit_packed(self, packed, rnd):
        """`zkhip_queue_submit_packed`: the assignment in the packed form (`pack_assignment`), widened on the device."""
        rb = self._rnd(rnd)
        packed = _u8(packed)
        ticket = C.c_uint64()
        self.ctx._check(self.ctx.lib.L.zkhip_queue_submit_packed(self.h, _ptr(packed), packed.size, _ptr(rb), C.byref(ticket)))
        return int(ticket.value)

    def submit_witness(self, plan, witness_bytes, rnd):
        """`zkhip_queue_submit_witness`: the assignment as the bytes of a ZoKrates `witness` file, ordered and checked on the device
        through `plan` (`Program.plan`, made before the queue was opened).  What the device finds wrong with the file fails the
        ticket at `collect`."""
        rb = self._rnd(rnd)
        wit = _u8(witness_bytes)
        ticket = C.c_uint64()
        self.ctx._check(self.ctx.lib.L.zkhip_queue_submit_witness(self.h, plan.h, _ptr(wit), wit.size, _ptr(rb), C.byref(ticket)))
        return int(ticket.value)

    def ready(self):
        """`zkhip_queue_ready`: would `collect` return without waiting for the device?  Never blocks; False on an empty queue."""
        out = C.c_int32()
        self.ctx._check(self.ctx.lib.L.zkhip_queue_ready(self.h, C.byref(out)))
        return bool(out.value)

    def collect(self, want_timings=False, want_inputs=False):
        """`zkhip_queue_collect`: (ticket, proof bytes) of the oldest proof in flight; blocks until it is done.  A proof that failed
        raises ZkhipError — its `ticket` attribute says which — and the others stay in flight.  `want_inputs`
        (`zkhip_queue_collect_inputs`): the public inputs (uint8[k*32]) follow the proof bytes — empty for a ticket that was not
        submitted as a witness file."""
        out = np.zeros(self.proof_bytes, dtype=np.uint8)
        ticket = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        tm = Timings()
        L = self.ctx.lib.L
        try:
            if want_inputs:
                cap = self.cs.l
                inputs = np.zeros(max(cap, 1) * 32, dtype=np.uint8)
                n_in = C.c_uint64()
                self.ctx._check(L.zkhip_queue_collect_inputs(self.h, C.byref(ticket), _ptr(out), _ptr(inputs), cap, C.byref(n_in), C.byref(tm)),
                                lambda: [out.tobytes()])
            else:
                self.ctx._check(L.zkhip_queue_collect(self.h, C.byref(ticket), _ptr(out), C.byref(tm)), lambda: [out.tobytes()])
        except ZkhipError as e:
            e.ticket = None if ticket.value == 0xFFFFFFFFFFFFFFFF else int(ticket.value)
            raise
        res = (int(ticket.value), out.tobytes())
        if want_inputs:
            res += (inputs[:32 * n_in.value].copy(),)
        return res + (tm.as_dict(),) if want_timings else res

    def close(self):
        """`zkhip_queue_close`: waits for what is in flight, drops it, and gives the context back."""
        if self.h:
            self.ctx.lib.L.zkhip_queue_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- ZoKrates' own files (N1): host only ----
class Program:
    """`zkhip_prog`: a ZoKrates `out` file parsed into the R1CS in ark variable order (no GPU involved)."""

    def __init__(self, data, library=None):
        self.lib = library or default_library()
        data = _u8(data)
        self.h = C.c_void_p()
        rc = self.lib.L.zkhip_prog_parse(_ptr(data), data.size, C.byref(self.h))
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_last_error(None).decode())
        d = np.zeros(8, dtype=np.uint64)
        self.lib.L.zkhip_prog_dims(self.h, _ptr(d))
        self.curve_id, self.n, self.l, self.w, self.return_count, self.n_public_args, self.nnz = (int(x) for x in d[:7])
        self.m = self.l + self.w

    def mats(self):
        """[(rowptr u64[n+1], col u32[nnz], val u8[nnz*32])] for A, B, C — copies."""
        out = []
        for k in range(3):
            rp, col, val = C.c_void_p(), C.c_void_p(), C.c_void_p()
            self.lib.L.zkhip_prog_matrix(self.h, k, C.byref(rp), C.byref(col), C.byref(val))
            rpa = np.ctypeslib.as_array(C.cast(rp, C.POINTER(C.c_uint64)), (self.n + 1,)).copy()
            nnz = int(rpa[-1])
            if nnz:
                cola = np.ctypeslib.as_array(C.cast(col, C.POINTER(C.c_uint32)), (nnz,)).copy()
                vala = np.ctypeslib.as_array(C.cast(val, C.POINTER(C.c_uint8)), (nnz * 32,)).copy()
            else:
                cola, vala = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
            out.append((rpa, cola, vala))
        return out

    def variable_order(self):
        ids = C.c_void_p()
        self.lib.L.zkhip_prog_variable_order(self.h, C.byref(ids))
        return np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_int64)), (self.m,)).copy()

    def constraint_system(self, ctx):
        """Upload to the GPU (`zkhip_prog_r1cs_load`)."""
        cs = ConstraintSystem.__new__(ConstraintSystem)
        cs.ctx, cs.curve_id, cs.n, cs.l, cs.w, cs.m = ctx, self.curve_id, self.n, self.l, self.w, self.m
        cs.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_prog_r1cs_load(ctx.h, self.h, C.byref(cs.h)))
        return cs

    def plan(self, ctx, cs):
        """`zkhip_wplan_create`: this program's column order resident on `ctx`, for `Context.upload_witness` and
        `ProofQueue.submit_witness` over `cs`.  Raises ZkhipError (BAD_ARG) for a program the device route cannot take (a repeated
        parameter, an output without a column): such callers keep `assignment`."""
        return WitnessPlan(ctx, self, cs)

    def exec_plan(self, ctx, cs, data):
        """`zkhip_xplan_create`: this program's statements compiled for the device, for `Context.compute_witness`.  `data`: the same
        `out` bytes the program was parsed from.  Raises ZkhipError (BAD_ARG) for a program that keeps the host interpreter (a solver
        the device does not run, a read before definition)."""
        return ExecPlan(ctx, self, cs, data)

    def assignment(self, witness_bytes):
        """(z uint8[m*32] in ark order, inputs uint8[k*32] = public_inputs_values) from a ZoKrates `witness` file."""
        wit = _u8(witness_bytes)
        z = np.zeros(self.m * 32, dtype=np.uint8)
        cap = self.n_public_args + wit.size // 40 + 1
        inputs = np.zeros(cap * 32, dtype=np.uint8)
        n_in = C.c_uint64()
        rc = self.lib.L.zkhip_prog_assignment(self.h, _ptr(wit), wit.size, _ptr(z), _ptr(inputs), cap, C.byref(n_in))
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_last_error(None).decode())
        return z, inputs[:32 * n_in.value].copy()

    def assignment_packed(self, witness_bytes):
        """`zkhip_prog_assignment_packed`: (the packed form of z, inputs) — `pack_assignment(self.assignment(w)[0])` without the
        caller holding the m x 32 B in between."""
        wit = _u8(witness_bytes)
        pcap = pack_bound(self.m, self.lib)
        packed = np.zeros(pcap, dtype=np.uint8)
        cap = self.n_public_args + wit.size // 40 + 1
        inputs = np.zeros(cap * 32, dtype=np.uint8)
        n_in, n_packed = C.c_uint64(), C.c_uint64()
        rc = self.lib.L.zkhip_prog_assignment_packed(self.h, _ptr(wit), wit.size, _ptr(packed), pcap, C.byref(n_packed), _ptr(inputs), cap, C.byref(n_in))
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_last_error(None).decode())
        return packed[:n_packed.value].copy(), inputs[:32 * n_in.value].copy()

    def close(self):
        if self.h:
            self.lib.L.zkhip_prog_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WitnessBatch:
    """What `Context.compute_witness` returns."""

    def close(self):
        for z in self.assignments:
            if z is not None:
                z.close()


class ExecPlan:
    """`zkhip_xplan`: the statements of one program compiled for the device, on one context (`Program.exec_plan`)."""

    DIMS = ("n_args", "n_statements", "n_defines", "n_checks", "n_directives", "n_entries", "n_extra", "store_bytes")

    def __init__(self, ctx, prog, cs, data):
        self.ctx = ctx
        data = _u8(data)
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_xplan_create(ctx.h, prog.h, cs.h, _ptr(data), data.size, C.byref(self.h)))
        d = np.zeros(8, dtype=np.uint64)
        ctx.lib.L.zkhip_xplan_dims(self.h, _ptr(d))
        self.dims = tuple(int(x) for x in d)
        for k, v in zip(self.DIMS, self.dims):
            setattr(self, k, v)
        self.n_inputs = prog.n_public_args + prog.return_count
        self.file_bytes = 8 + 40 * self.n_entries

    def levels(self):
        """`zkhip_xplan_levels`: (levels, instructions of the widest level, instructions in all, levels of fewer than 64)."""
        d = np.zeros(4, dtype=np.uint64)
        self.ctx._check(self.ctx.lib.L.zkhip_xplan_levels(self.h, _ptr(d)))
        return tuple(int(x) for x in d)

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_xplan_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WitnessPlan:
    """`zkhip_wplan`: the id -> column tables of one program on one context (`Program.plan`)."""

    def __init__(self, ctx, prog, cs):
        self.ctx = ctx
        self.n_inputs = prog.n_public_args + prog.return_count
        self.h = C.c_void_p()
        ctx._check(ctx.lib.L.zkhip_wplan_create(ctx.h, prog.h, cs.h, C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.lib.L.zkhip_wplan_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_program(curve_id, n, m, mats, ids=None, args=((1, False),), return_count=0, library=None):
    """`zkhip_prog_write`: the R1CS `mats` (as for ConstraintSystem) as the bytes of a ZoKrates `out` program.  ids[j] = the
    ZoKrates variable id of column j (default j: column 0 = ~one, column j = _{j-1}); args = [(id, private)]."""
    lib = library or default_library()
    ids = np.arange(m, dtype=np.int64) if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
    if ids.size != m:
        raise ValueError("one id per column")
    keep, a, nnz = [], [], 0
    for rp, col, val in mats:
        rp = np.ascontiguousarray(rp, dtype=np.uint64); col = np.ascontiguousarray(col, dtype=np.uint32); val = _u8(val)
        if rp.size != n + 1 or val.size != col.size * 32:
            raise ValueError("CSR shape mismatch")
        keep += [rp, col, val]
        a += [_ptr(rp), _ptr(col), _ptr(val)]
        nnz += int(col.size)
    arg_ids = np.asarray([i for i, _ in args], dtype=np.int64)
    arg_priv = np.asarray([1 if p else 0 for _, p in args], dtype=np.uint8)
    bound = C.c_uint64()
    lib.L.zkhip_prog_write_bound(n, nnz, len(args), C.byref(bound))
    out = np.empty(bound.value, dtype=np.uint8)
    ln = C.c_uint64()
    rc = lib.L.zkhip_prog_write(curve_id, n, m, *a, _ptr(ids), _ptr(arg_ids), _ptr(arg_priv), len(args), return_count, _ptr(out), bound.value, C.byref(ln))
    if rc != 0:
        raise ZkhipError(rc, lib.L.zkhip_last_error(None).decode())
    return out[:ln.value]


def write_witness(ids, z):
    """`Witness::write` (/root/reference/zokrates_ast/src/ir/witness.rs:44-53): usize count, then (isize id, 32-byte canonical
    LE value) in ascending signed-id order (the BTreeMap's).  ids[j] names entry j of z (uint8[m*32])."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    z = _u8(z, ids.size * 32).reshape(-1, 32)
    order = np.argsort(ids, kind="stable")
    rec = np.zeros(ids.size, dtype=[("id", "<i8"), ("v", "u1", 32)])
    rec["id"] = ids[order]
    rec["v"] = z[order]
    return np.concatenate([np.frombuffer(int(ids.size).to_bytes(8, "little"), dtype=np.uint8), rec.view(np.uint8).reshape(-1)])


class Multi:
    """`zkhip_multi`: ONE proof across several GPUs of this process (no collective library, no Python in the data path):
    member k holds shard k of n of the key and a replica of the constraint system.  `devices` may repeat a device."""

    def __init__(self, devices, library=None):
        self.lib = library or default_library()
        self.h = C.c_void_p()
        dev = np.asarray(list(devices), dtype=np.int32)
        rc = self.lib.L.zkhip_ctx_create_multi(_ptr(dev), int(dev.size), C.byref(self.h))
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_last_error(None).decode())
        self.curve_id = None
        self.m = None

    def _check(self, rc):
        if rc != 0:
            raise ZkhipError(rc, self.lib.L.zkhip_multi_last_error(self.h).decode())

    def __len__(self):
        return int(self.lib.L.zkhip_multi_size(self.h))

    def member_context(self, k=0):
        """A borrowed `Context` of member k (do not close it): e.g. to run the setup on the same device."""
        ctx = Context.__new__(Context)
        ctx.lib = self.lib
        ctx.h = C.c_void_p(self.lib.L.zkhip_multi_ctx(self.h, k))
        ctx.close = lambda: None
        return ctx

    def use_rccl(self, on=True):
        """`zkhip_multi_use_rccl`: exchange the members' shares with an RCCL all-gather instead of through host memory."""
        self._check(self.lib.L.zkhip_multi_use_rccl(self.h, 1 if on else 0))

    def exchange(self):
        return self.lib.L.zkhip_multi_exchange(self.h).decode()

    def load_constraint_system(self, curve_id, n, l, w, mats):
        keep = []
        args = []
        for rp, col, val in mats:
            rp = np.ascontiguousarray(rp, dtype=np.uint64); col = np.ascontiguousarray(col, dtype=np.uint32); val = _u8(val)
            keep += [rp, col, val]
            args += [_ptr(rp), _ptr(col), _ptr(val)]
        self._check(self.lib.L.zkhip_multi_r1cs_load(self.h, curve_id, n, l, w, *args))
        self.curve_id, self.m = curve_id, l + w
        self.domain = 1
        while self.domain < n + l:
            self.domain *= 2

    def load_proving_key(self, curve_id, pk_bytes, scheme="g16"):
        b = _u8(pk_bytes)
        fn = self.lib.L.zkhip_multi_pk_load_gm17 if scheme == "gm17" else self.lib.L.zkhip_multi_pk_load_g16
        self._check(fn(self.h, curve_id, _ptr(b), b.size))
        self.curve_id = curve_id

    def load_proving_key_replicas(self, curve_id, pk_bytes):
        """Throughput mode: the whole Groth16 key on every member (`zkhip_multi_pk_load_g16_replicas`)."""
        b = _u8(pk_bytes)
        self._check(self.lib.L.zkhip_multi_pk_load_g16_replicas(self.h, curve_id, _ptr(b), b.size))
        self.curve_id = curve_id

    def bind(self, pk_bytes):
        """`zkhip_multi_bind`: the members' keys bound to the members' constraint system (one member computes the bound bases from
        the key file, every member installs its index ranges)."""
        b = _u8(pk_bytes)
        self._check(self.lib.L.zkhip_multi_bind(self.h, _ptr(b), b.size))

    def unbind(self):
        self._check(self.lib.L.zkhip_multi_unbind(self.h))

    def transform_split(self, on=None):
        """`zkhip_multi_transform_split`: let bound members split a proof's witness map (None: only report).  Returns the previous setting."""
        return bool(self.lib.L.zkhip_multi_transform_split(self.h, -1 if on is None else int(bool(on))))

    def last_split(self):
        return bool(self.lib.L.zkhip_multi_last_split(self.h))

    def transform_shard(self, on=None):
        """`zkhip_multi_transform_shard`: let proofs over an unbound Groth16 key shard their witness map's domain across the members
        (None: only report; off by default).  Returns the previous setting."""
        return bool(self.lib.L.zkhip_multi_transform_shard(self.h, -1 if on is None else int(bool(on))))

    def last_shard(self):
        """Members the transforms of the last `ntt` / `witness_map` / `prove_*` were sharded over (0: they were not)."""
        return int(self.lib.L.zkhip_multi_last_shard(self.h))

    def ntt(self, curve_id, data, direction):
        """`zkhip_multi_ntt`: `Context.ntt` with the domain sharded across the members where the plan allows it."""
        d = np.array(_u8(data), dtype=np.uint8, copy=True)
        n = d.size // 32
        logn = n.bit_length() - 1
        if n == 0 or (1 << logn) != n:
            raise ValueError("NTT size must be a power of two")
        code = {"fft": 0, "ifft": 1, "coset_fft": 2, "coset_ifft": 3}[direction]
        self._check(self.lib.L.zkhip_multi_ntt(self.h, curve_id, logn, code, _ptr(d)))
        return d

    def witness_map(self, z):
        """`zkhip_multi_witness_map` over the loaded constraint system: h as N x 32 bytes, natural order, as
        `ConstraintSystem.witness_map` returns it."""
        z = _u8(z, self.m * 32)
        out = np.zeros(self.domain * 32, dtype=np.uint8)
        self._check(self.lib.L.zkhip_multi_witness_map(self.h, _ptr(z), _ptr(out)))
        return out

    def prove_g16_batch(self, zs, rss):
        """Independent proofs dealt over the members (`zkhip_prove_g16_multi_batch`): zs = list of host assignments,
        rss = list of (r, s).  Returns (list of proof bytes, timings dict)."""
        nb = FQ_BYTES[self.curve_id]
        count = len(zs)
        z = np.ascontiguousarray(np.concatenate([_u8(a, self.m * 32) for a in zs])) if count else np.zeros(1, dtype=np.uint8)
        rs = np.frombuffer(b"".join(int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little") for r, s in rss) or b"\0", dtype=np.uint8)
        out = np.zeros(max(count, 1) * (8 * nb + 3), dtype=np.uint8)
        tm = Timings()
        self._check(self.lib.L.zkhip_prove_g16_multi_batch(self.h, count, _ptr(z), _ptr(rs), _ptr(out), C.byref(tm)))
        pb = 8 * nb + 3
        return [out[i * pb:(i + 1) * pb].tobytes() for i in range(count)], tm.as_dict()

    def prove_g16(self, z, r, s, want_timings=False):
        nb = FQ_BYTES[self.curve_id]
        z = _u8(z, self.m * 32)
        rb = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8)
        sb = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)
        out = np.zeros(8 * nb + 3, dtype=np.uint8)
        tm = Timings()
        self._check(self.lib.L.zkhip_prove_g16_multi(self.h, _ptr(z), _ptr(rb), _ptr(sb), _ptr(out), C.byref(tm)))
        return (out.tobytes(), tm.as_dict()) if want_timings else out.tobytes()

    def prove_gm17(self, z, d1, d2, r, want_timings=False):
        nb = FQ_BYTES[self.curve_id]
        z = _u8(z, self.m * 32)
        rnd = _rnd96(d1, d2, r)
        out = np.zeros(8 * nb + 3, dtype=np.uint8)
        tm = Timings()
        self._check(self.lib.L.zkhip_prove_gm17_multi(self.h, _ptr(z), _ptr(rnd), _ptr(out), C.byref(tm)))
        return (out.tobytes(), tm.as_dict()) if want_timings else out.tobytes()

    def close(self):
        if self.h:
            self.lib.L.zkhip_multi_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
