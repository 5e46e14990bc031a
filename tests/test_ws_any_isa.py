"""Static facts of mlp_ws_any_kernel — the weight-stationary kernel's dense pairs for segments of any length (csrc/mlp_ws.hip) — from
the code object's metadata of a device-only cross-compile (no GPU): every instantiation (three / two layers, plain message launch /
fused MP layer, tracked / certified) uses no scratch, spills no scalar and no vector register, stays inside the 256 registers of two
waves per SIMD, and carries the range tracker (v_max3_f32) exactly when it is a tracked one."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphs4cfd_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def mangled(n_layers, node, track):
    return f"mlp_ws_any_kernelILi{n_layers}ELb{int(node)}ELb{int(track)}EE"


FORMS = [(nl, node, track) for nl in (3, 2) for node in (False, True) for track in (True, False)]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("ws_any_isa") / "mlp_ws_any.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-DG4C_WS_ISA_ONLY=3", "-S",
                    os.path.join(CSRC, "mlp_ws.hip"), "-o", out], check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def metadata(text, key):
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if key in name:
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size):\s+(\d+)", block)}
    raise AssertionError(f"no kernel {key}")


def body(text, key):
    start = next(m.start() for m in re.finditer(r"^(_Z\w+):", text, re.M) if key in m.group(1))
    return text[start:text.index("s_endpgm", start)]


@pytest.mark.parametrize("n_layers,node,track", FORMS)
def test_instantiations_spill_nothing(asm, n_layers, node, track):
    key = mangled(n_layers, node, track)
    md = metadata(asm, key)
    print(key, md)
    assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 255, md
    assert ("v_max3_f32" in body(asm, key)) == track          # the range tracker: one per converted pair, tracked instantiations only


def test_only_these_forms_are_instantiated(asm):
    names = set(re.findall(r"\.name:\s+(_Z\S+)", asm))
    assert len(names) == len(FORMS) and all(any(mangled(*f) in n for f in FORMS) for n in names), names
