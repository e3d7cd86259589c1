"""CPU: the LDS layout the panel kernel carves and its launcher sizes (PanelLds, kernels_common.h) against the carve as
plain arithmetic -- evaluated by the compiler, no GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANEL, MAX_K = 64, 8


def _carve(qcap, mix, mirror):
    """q[qcap] | a[2][64] | diagonal tiles[2][64 x 64] | off-diagonal tile[64 x 64] | mixture scratch | ed[2][64] | s[qcap]"""
    off = {"q": 0, "a": qcap}
    off["diag_tiles"] = off["a"] + 2 * PANEL
    off["offdiag_tile"] = off["diag_tiles"] + 2 * PANEL * PANEL
    off["mix"] = off["offdiag_tile"] + PANEL * PANEL
    off["ed"] = off["mix"] + (5 * PANEL * MAX_K if mix else 0)
    off["s"] = off["ed"] + 2 * PANEL
    # what the launcher reserved before PanelLds: panel_lds_floats(qcap, true) + kMixLdsFloats + panel_mirror_lds_floats(qcap)
    total = (qcap + 2 * PANEL + 2 * PANEL * PANEL + PANEL * PANEL) + (5 * PANEL * MAX_K if mix else 0) + \
            ((2 * PANEL + qcap) if mirror else 0)
    return off, total


def test_panel_lds_layout_equals_the_plain_carve(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    lines = ['#include "kernels_common.h"', "using viprs::PanelLds;"]
    for qcap in (256, 320, 1856, 13440):
        for mix in (False, True):
            for mirror in (False, True):
                off, total = _carve(qcap, mix, mirror)
                L = f"PanelLds({qcap}, {str(mix).lower()}, {str(mirror).lower()})"
                lines.append(f'static_assert({L}.total_floats() == {total}, "total {qcap} {mix} {mirror}");')
                for name, o in off.items():
                    lines.append(f'static_assert({L}.{name}() == {o}, "{name} {qcap} {mix} {mirror}");')
    src = tmp_path / "panel_lds_check.hip"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "viprs_amd", "csrc"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
