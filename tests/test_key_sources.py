"""The one parser per proving-key format (PkLoader::parse_g16 / parse_gm17 in csrc/core.cuh, shared by key load and bind-from-file),
checked by a stand-alone host program: no device, no context, nothing loaded into this process."""
import os
import subprocess


def test_key_sources_host(tmp_path):
    """tests/host/key_sources.cpp built for the emulator target under ASan + UBSan, as tests/host/slot_sums_layout.cpp is: every pointer,
    count, shift and index of the KeySources returned for key files of both schemes and both point sizes, and every prefix, trailing
    byte, overwritten length field and file of the other scheme refused."""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "key_sources")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DZK_EMU", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(here, "..", "zokrates_amd", "csrc"), os.path.join(here, "host", "key_sources.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
