"""Static facts of mlp_ws_pre_kernel — the weight-stationary kernel's "first layer precomputed" form (csrc/mlp_ws.hip) — from the code
object's metadata of a device-only cross-compile (no GPU): the two instantiations, dense pairs and table-driven tiles, use no scratch,
spill no scalar and no vector register and stay inside the 256 registers of two waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphs4cfd_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"dense": "mlp_ws_pre_kernelILb1EE", "tiles": "mlp_ws_pre_kernelILb0EE"}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("ws_pre_isa") / "mlp_ws_pre.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-DG4C_WS_ISA_ONLY=2", "-S",
                    os.path.join(CSRC, "mlp_ws.hip"), "-o", out], check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return out, open(out).read()


def metadata(text, key):
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if key in name:
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size):\s+(\d+)", block)}
    raise AssertionError(f"no kernel {key}")


@pytest.mark.parametrize("form", sorted(KERNELS))
def test_new_instantiations_spill_nothing(asm, form):
    _, text = asm
    md = metadata(text, KERNELS[form])
    print(form, md)
    assert md["private_segment_fixed_size"] == 0 and md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 255, md


def test_only_the_two_forms_are_instantiated(asm):
    _, text = asm
    names = set(re.findall(r"\.name:\s+(_Z\S+)", text))
    assert len(names) == 2 and all(any(k in n for k in KERNELS.values()) for n in names), names
