"""Static facts of the 64-row tile form of mlp_bx6_kernel's launch shapes (include/g4c.h g4c_mlp_tile_form; mlp_fused.hip tile_go_rows64),
from the cross-compiled assembly (no GPU), as tests/test_tile_isa.py reads them for form 0.  64-row tiles (RT = 2): no spills, no scratch,
at most 168 vector registers (three workgroups per CU) and 53 KB of LDS.  Form 0 itself — the instantiations tests/test_tile_isa.py names —
is still there within its bounds.  (A five-workgroup form of the 32-row tiles, at most 96 registers, was measured and is not shipped:
scripts/variants/r23_tile_five_workgroups.patch; nothing to check here.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphs4cfd_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# template arguments RT, VEC, FULL, SP, SAVE, RD6 | TRACK | SH in the mangled name
FORM = {32: "mlp_bx6_kernelILi1ELb1ELb1ELi2ELb0ELi2E", 64: "mlp_bx6_kernelILi2ELb1ELb1ELi2ELb0ELi2E"}
TRACKED, CERTIFIED = "Lb1E", "Lb0E"
# TileShape<ID, N_SRC, IDX0, N_NAR, N_LAYERS, N_HEADS>
NODE = {f"node-{nl}-{nh}": f"9TileShapeILi1ELi2ELb0ELi0ELi{nl}ELi{nh}EE" for nl in (2, 3) for nh in (0, 2)}
UP = {f"up-{nl}-{nh}": f"9TileShapeILi2ELi2ELb1ELi1ELi{nl}ELi{nh}EE" for nl in (2, 3) for nh in (0, 2)}
DOWN = {f"down-{nl}-0": f"9TileShapeILi3ELi1ELb0ELi1ELi{nl}ELi0EE" for nl in (2, 3)}
SHAPES = {**NODE, **UP, **DOWN}


def plain(shape):
    return "N4g4cm" + SHAPES[shape] + "E"


# what tile_go_rows64 launches: (shape, tracker) — the UpMP shape has no tracker-free form, the DownMP shape no 64-row form
ROWS64 = [(s, t) for s in sorted({**NODE, **UP}) for t in (TRACKED, CERTIFIED) if t == TRACKED or s in NODE]
# tests/test_tile_isa.py's cases
FORM0 = [(s, t) for s in sorted(NODE) + ["up-3-0", "up-3-2", "down-3-0"] for t in (TRACKED, CERTIFIED) if t == TRACKED or s in NODE]
KEYS = r"sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size|group_segment_fixed_size"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("tile_forms_isa") / "mlp_fused.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-DG4C_TILE_ISA_ONLY", "-S",
                    os.path.join(CSRC, "mlp_fused.hip"), "-o", out], check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def metadata(text, key):
    """The .amdgpu_metadata entry of the one kernel whose mangled name contains `key`."""
    found = []
    for block in text.split("  - .agpr_count:")[1:]:
        if key in re.search(r"\.name:\s+(\S+)", block).group(1):
            found.append({k: int(v) for k, v in re.findall(rf"\.({KEYS}):\s+(\d+)", block)})
    assert len(found) == 1, (key, len(found))
    return found[0]


def no_spill(md):
    return md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0


@pytest.mark.parametrize("shape,track", ROWS64)
def test_64_row_instantiations(asm, shape, track):
    md = metadata(asm, FORM[64] + track + plain(shape))
    print(f"{shape}, {'tracked' if track == TRACKED else 'certified'}, 64 rows: {md}")
    assert no_spill(md), md
    assert md["vgpr_count"] <= 168, md
    assert md["group_segment_fixed_size"] <= 54272, md


@pytest.mark.parametrize("shape,track", FORM0)
def test_form_0_instantiations_stay(asm, shape, track):
    md = metadata(asm, FORM[32] + track + plain(shape))
    assert no_spill(md), md
    assert md["vgpr_count"] <= 128, md


def test_64_row_tiles_exist_for_the_shipped_shapes_only(asm):
    """RT = 2 is admitted for the shaped f16x3 inference instantiations alone (the kernel's static_assert), and built for the shapes
    whose headline launches it won: no generic one, none of the DownMP shape."""
    names = [n for n in re.findall(r"\.name:\s+(\S+)", asm) if FORM[64] in n]
    assert len(names) == len(ROWS64)
    assert not any("TileShapeGeneric" in n or any(d in n for d in DOWN.values()) for n in names)
