"""The C ABI boundary: libzkhip.so (the real gfx950 build) loads without a GPU and exports every function that
include/zkhip.h declares; the ctypes binding covers all of them; without a device the library fails loudly instead of
falling back to anything."""
import ctypes
import os
import re

import pytest

from zokrates_amd import build as zbuild
from zokrates_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zkhip_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    return zbuild.build_lib()          # hipcc cross-compiles for gfx950 without a GPU (incremental)


def test_header_symbols_are_exported(lib_path):
    names = declared_functions()
    assert len(names) >= 25
    dll = ctypes.CDLL(lib_path)
    missing = [n for n in names if not hasattr(dll, n)]
    assert not missing, missing


def test_binding_covers_the_header():
    assert sorted(native.Library.SYMBOLS) == declared_functions()


def test_matvec_shape_query_is_declared_bound_and_refuses_null():
    """zkhip_r1cs_matvec_shape (what tests/test_matvec_widths.py asserts its widths through) is in the header and in the binding, and
    answers ZKHIP_ERR_BAD_ARG, not a crash, for a null handle or a null result."""
    import ctypes as C
    from emu_util import emu_library
    assert "zkhip_r1cs_matvec_shape" in declared_functions() and "zkhip_r1cs_matvec_shape" in native.Library.SYMBOLS
    fn = emu_library().L.zkhip_r1cs_matvec_shape
    lanes, a, b = (C.c_int32 * 3)(), C.c_uint64(), C.c_uint64()
    assert fn(None, lanes, C.byref(a), C.byref(b)) == -1
    ctx = native.Context(0, emu_library())
    rp = [0, 1]
    one = (1).to_bytes(32, "little")
    cs = native.ConstraintSystem(ctx, 0, 1, 1, 1, [(rp, [0], one), (rp, [1], one), (rp, [1], one)])
    assert fn(cs.h, None, C.byref(a), C.byref(b)) == -1 and fn(cs.h, lanes, None, C.byref(b)) == -1 and fn(cs.h, lanes, C.byref(a), None) == -1
    assert cs.matvec_shape() == ((1, 1, 1), 0, 0)
    cs.close()
    ctx.close()


def test_no_cpu_fallback(lib_path):
    """On a machine without a GPU the product library refuses to create a context (ZKHIP_ERR_DEVICE)."""
    lib = native.Library(lib_path)
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(native.ZkhipError) as e:
        native.Context(0, lib)
    assert e.value.code == -4


def test_rust_bindings_and_integration_excerpt_follow_the_header():
    """The Rust crate cannot be compiled here, so at least its `extern "C"` block is held against include/zkhip.h
    mechanically: every function it declares exists in the header with the same number of parameters, and every function the
    INTEGRATION.md §2 excerpt shows is declared by the crate (the two had drifted in round 2)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "zkhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(?:int32_t|void|const char\*|zkhip_ctx\*)\s+(zkhip_\w+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1

    def rust_fns(text):
        out = {}
        for m in re.finditer(r"pub fn (zkhip_\w+)\s*\((.*?)\)\s*(?:->\s*[\w*\s]+)?;", text, flags=re.S):
            args = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).strip()
            out[m.group(1)] = 0 if not args else args.count(":")
        return out

    ffi = rust_fns(open(os.path.join(root, "integration", "zokrates_hip", "src", "ffi.rs")).read())
    assert len(ffi) >= 25
    for name, nargs in ffi.items():
        assert name in protos, name + " is not in include/zkhip.h"
        assert protos[name] == nargs, (name, protos[name], nargs)
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    excerpt = rust_fns(doc[doc.index("## 2."):doc.index("## 3.")])
    assert excerpt and set(excerpt) <= set(ffi), set(excerpt) - set(ffi)
    for name, nargs in excerpt.items():
        assert ffi[name] == nargs, name


def test_device_pci_bus_id_on_the_emulator_and_without_a_gpu(lib_path):
    """zkhip_device_pci_bus_id: what ties a device ordinal to /sys/bus/pci/devices/<address> (NUMA node, hwmon).  The emulator's one
    "device" answers a fixed address; the product library without a GPU answers an error, not a made-up address."""
    from emu_util import emu_library
    assert emu_library().device_pci_bus_id(0) == "0000:00:00.0"
    lib = native.Library(lib_path)
    if lib.device_count() == 0:
        assert lib.device_pci_bus_id(0) is None
