"""The state of a device buffer around a failed allocation (viprs_amd/csrc/dev_buf.h), checked on the host with stand-in
allocators: a failure leaves the buffer empty, so the retry that `viprs_genotypes_ld`'s out-of-memory message recommends
allocates again and never launches on a null pointer.  Needs no device: tests/dev_buf_state.cpp is a host program."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "viprs_amd", "csrc")


def test_failed_allocation_leaves_the_buffer_empty(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    exe = str(tmp_path / "dev_buf_state")
    r = subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                        os.path.join(HERE, "dev_buf_state.cpp"),
                        "-o", exe, "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "dev_buf_state OK" in r.stdout, r.stdout + r.stderr


def test_every_grown_buffer_of_the_ld_call_goes_through_reserve():
    """No `n < need` test in front of an allocation in the LD path: the capacity alone must not decide."""
    src = open(os.path.join(CSRC, "abi_genotypes.hip")).read()
    body = src[src.index("int viprs_genotypes_ld("):src.index("int viprs_genotypes_last_ld_ms(")]
    tables = src[src.index("int ensure_ld_tables("):src.index("int enqueue_ld(")]
    for text in (body, tables):
        assert not re.search(r"\.n\s*<", text) and ".alloc(" not in text
    for buf in ("d_right_end", "d_indptr", "d_w", "d_pairs", "d_ld_out"):
        assert f"G->{buf}.reserve(" in body, buf
    # on every path after the first upload is queued the stream is drained before the host vectors go out of scope
    tail = body[body.index("enqueue_ld("):]
    assert tail.index("hipStreamSynchronize(G->stream)") < tail.index("return")
    # and internal.h has no second definition of the buffer
    assert "struct DevBuf" not in open(os.path.join(CSRC, "internal.h")).read()
