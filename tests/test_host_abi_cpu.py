"""csrc/host_abi.cpp, csrc/measure_report.cpp and csrc/host_pool.h are host code: with csrc/fold.cpp they make a shared library under the
host compiler alone, with no symbol left undefined -- no HIP call and no reference to the generator (csrc/engine.hip) in them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grav1synth_amd", "csrc")


def test_the_host_abi_links_without_hip(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    so = tmp_path / "libg1s_host.so"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wl,--no-undefined", "-o", str(so),
                           os.path.join(CSRC, "fold.cpp"), os.path.join(CSRC, "host_abi.cpp"), os.path.join(CSRC, "measure_report.cpp"), "-lpthread"])
    L = C.CDLL(str(so))
    for name in ("g1s_fold_new", "g1s_shard_merge", "g1s_record_init", "g1s_latest_from_records", "g1s_parse_tbl", "g1s_usable_cpus",
                 "g1s_last_global_error", "g1s_format_measure", "g1s_measure_sum_scales"):
        assert hasattr(L, name), name
    L.g1s_usable_cpus.restype = C.c_uint
    assert L.g1s_usable_cpus() >= 1


@pytest.mark.parametrize("name", ["host_abi.cpp", "host_pool.h", "measure_report.cpp"])
def test_the_host_files_include_no_hip_header(name):
    text = open(os.path.join(CSRC, name)).read()
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', text, flags=re.M)
    assert includes and not [i for i in includes if i.startswith("hip/") or i.endswith(".hip.h")], includes
    # (frame_op.h and latest_dev.h bring the runtime's header in under hipcc: the host files stay clear of them too)
    assert not {"frame_op.h", "latest_dev.h"} & set(includes), includes
