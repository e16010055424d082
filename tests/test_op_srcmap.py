"""The source map of an updatable face-weight operator (csrc/op_pack.hip, ``PackOptions::updatable``) without a GPU:
tools/sanitize/pack_srcmap.cpp -- a program of its own that links the host-only packer -- packs the shapes of
tests/test_gpu_face_update.py (a 5x4x3 box, a 13^3 box with shuffled and flipped faces, the reference's triangles, a ring
with a hub whose row spills into the CSR tail, ``ell_cap = 2``, a halo plane, cells without faces) from 1, 3 and 7 build
threads and decodes every slot and tail entry back to its face and side; the records must be those of a plain pack under
``spmv_dict = 0`` byte for byte, and a pack without the flag must carry no map.  Built once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer; both binaries are run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a_box_5x4x3", "b_box_13_shuffled_flipped", "c_triangles_square_nb", "d_ring_200_and_hub", "d2_box_13_ell_cap_2",
         "e_box_5x4x3_last_plane_halo", "f_three_cells_no_faces")


def _build(exe, extra):
    csrc = os.path.join(ROOT, "stormruler_amd", "csrc")
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tools", "sanitize", "pack_srcmap.cpp"),
                           "-x", "c++", os.path.join(csrc, "op_pack.hip"), "-o", str(exe), "-lpthread"], capture_output=True, text=True)


def _run_and_check(exe):
    env = {k: v for k, v in os.environ.items() if k not in ("STORM_HIP_BUILD_THREADS", "STORM_HIP_BUILD_MIN_CHUNK")}
    p = subprocess.run([str(exe), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert lines[-1] == "srcmap: ok"
    for threads in ("1", "3", "7"):
        for case in CASES:
            assert any(ln.startswith(f"{case} threads={threads}:") and ln.endswith(" ok") for ln in lines), (case, threads)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    return lines


def test_every_slot_decodes_to_its_face_and_side(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not available here")
    exe = tmp_path / "pack_srcmap"
    b = _build(exe, ["-Wall"])
    assert b.returncode == 0, b.stderr[-4000:]
    lines = _run_and_check(exe)
    # the shapes exercise what they are there for: a CSR tail (d, d2), none elsewhere
    tail = {ln.split()[0]: int(ln.split(",")[-1].split()[0]) for ln in lines if "threads=1:" in ln}
    assert tail["d_ring_200_and_hub"] > 100 and tail["d2_box_13_ell_cap_2"] > 2197
    assert tail["a_box_5x4x3"] == tail["c_triangles_square_nb"] == tail["e_box_5x4x3_last_plane_halo"] == 0


def test_the_same_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not available here")
    exe = tmp_path / "pack_srcmap_san"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    b = _build(exe, san + ["-static-libasan", "-static-libubsan"])  # (the runtimes inside the program where they exist as archives)
    if b.returncode != 0:
        b = _build(exe, san)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        pytest.skip("g++ with libasan / libubsan is not available here")
    assert b.returncode == 0, b.stderr[-4000:]
    _run_and_check(exe)
