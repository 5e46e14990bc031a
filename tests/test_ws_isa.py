"""Static facts of the headline step's mlp_ws_kernel instantiations, from the cross-compiled assembly (no GPU): no scalar-register
spills (they live in lanes of a vector register and come back as v_readlane in the pair loop), no scratch, at most 255 vector
registers, and no range tracker (v_max3_f32) in the certified instantiations."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphs4cfd_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# template arguments AGG, DIRECT, ADDS, SP, NL, XB16, AB16, NODE, DENSE, TRACK in the mangled name
DENSE, NODE = "ILb1ELb1ELb1ELi2ELi3ELb0ELb0ELb0ELb1E", "ILb1ELb1ELb1ELi2ELi3ELb0ELb0ELb1ELb0E"
TRACKED, CERTIFIED = "Lb1EE", "Lb0EE"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("ws_isa") / "mlp_ws.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-DG4C_WS_ISA_ONLY", "-S",
                    os.path.join(CSRC, "mlp_ws.hip"), "-o", out], check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return out, open(out).read()


def metadata(text, key):
    """The .amdgpu_metadata entry of the kernel whose mangled name contains `key`."""
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if key in name:
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size):\s+(\d+)", block)}
    raise AssertionError(f"no kernel {key}")


def body(text, key):
    start = next(m.start() for m in re.finditer(r"^(_Z\w+):", text, re.M) if key in m.group(1))
    return text[start:text.index("s_endpgm", start)]


@pytest.mark.parametrize("shape", [DENSE, NODE])
@pytest.mark.parametrize("track", [TRACKED, CERTIFIED])
def test_headline_instantiations_spill_nothing(asm, shape, track):
    _, text = asm
    md = metadata(text, shape + track)
    assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 255, md
    code = body(text, shape + track)
    assert "v_readlane_b32" not in code and "v_writelane_b32" not in code
    assert ("v_max3_f32" in code) == (track == TRACKED)          # one per converted pair, tracked instantiations only


def test_pair_loop_of_the_level1_launch(asm):
    """scripts/isa_count.py on the same file: the pair loop's instruction mix (2 876 instructions, 1 282 plain VALU, 494 SALU, 33
    v_readlane before the argument block / dense metas were reworked)."""
    path, _ = asm
    for track, vmax in ((TRACKED, 32), (CERTIFIED, 0)):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_count.py"), path, DENSE + track], check=True,
                             capture_output=True, text=True).stdout
        print(out)
        loop = int(re.search(r"main loop: (\d+) instructions", out).group(1))
        mfma = int(re.search(r"^\s+mfma\s+(\d+)", out, re.M).group(1))
        m = re.search(r"v_max3_f32\s+(\d+)", out)
        assert mfma == 192 and loop < 2500, out
        assert (int(m.group(1)) if m else 0) == vmax
