"""Static facts of mlp_bx6_kernel's launch shapes (mlp_common.h TileShapeNode / TileShapeUp / TileShapeDown), from the cross-compiled assembly (no GPU): no
spills, no scratch, at most 128 vector registers (four workgroups per CU, as the generic instantiation), no segment-reduction loop (its
mean is the only IEEE division of the kernel: the LayerNorm multiplies by a reciprocal square root), and fewer instructions than the
generic instantiation compiled in the same run."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphs4cfd_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# template arguments RT, VEC, FULL, SP, SAVE, RD6 | TRACK | SH in the mangled name
FORM = "mlp_bx6_kernelILi1ELb1ELb1ELi2ELb0ELi2E"
TRACKED, CERTIFIED = "Lb1E", "Lb0E"
GENERIC = "N4g4cm16TileShapeGenericE"
# TileShape<ID, N_SRC, IDX0, N_NAR, N_LAYERS, N_HEADS>: the node update (2 or 3 layers, 0 or 2 heads), three-layer UpMP and DownMP
SHAPES = {f"node-{nl}-{nh}": f"N4g4cm9TileShapeILi1ELi2ELb0ELi0ELi{nl}ELi{nh}EEE" for nl in (2, 3) for nh in (0, 2)}
SHAPES.update({f"up-3-{nh}": f"N4g4cm9TileShapeILi2ELi2ELb1ELi1ELi3ELi{nh}EEE" for nh in (0, 2)})
SHAPES["down-3-0"] = "N4g4cm9TileShapeILi3ELi1ELb0ELi1ELi3ELi0EEE"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("tile_isa") / "mlp_fused.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-DG4C_TILE_ISA_ONLY", "-S",
                    os.path.join(CSRC, "mlp_fused.hip"), "-o", out], check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    return open(out).read()


def metadata(text, key):
    """The .amdgpu_metadata entry of the kernel whose mangled name contains `key`."""
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if key in name:
            return {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size):\s+(\d+)", block)}
    raise AssertionError(f"no kernel {key}")


def instructions(text, key):
    start = next(m.start() for m in re.finditer(r"^(_Z\w+):", text, re.M) if key in m.group(1))
    body = text[start:text.index("s_endpgm", start)]
    return [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and ln.strip() and ln.strip()[0] not in ".;"]


# (a launch with a narrow block is never certified: the UpMP / DownMP shapes have no tracker-free form)
CASES = [(s, t) for s in sorted(SHAPES) for t in (TRACKED, CERTIFIED) if t == TRACKED or s.startswith("node")]


@pytest.mark.parametrize("shape,track", CASES)
def test_shaped_instantiations(asm, shape, track):
    key = FORM + track + SHAPES[shape]
    md = metadata(asm, key)
    assert md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 128, md
    code, generic = instructions(asm, key), instructions(asm, FORM + track + GENERIC)
    print(f"{shape} (layers, heads), {'tracked' if track == TRACKED else 'certified'}: {len(code)} instructions, generic {len(generic)}; "
          f"{md['vgpr_count']} VGPRs")
    assert "v_div_scale_f32" not in code          # the segment mean of the aggregation on load: not instantiated
    assert "v_div_scale_f32" in generic           # (what the assertion above looks for is there where the path is)
    assert len(code) < len(generic)
