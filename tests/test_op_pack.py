"""The host-only half of the operator build (csrc/op_pack.hip) without a GPU: tools/sanitize/pack_digest.cpp packs a fixed
corpus -- boxes that take every record format, a slab with halo columns (mixed and not), a renumbered box, distinct
weights, CSR operators with a tail, faces with a 300-entry row, the geometric entry point, an empty operator, each at
spmv_dict 0 to 4 -- and prints one digest per case over every scalar and every byte of the image.  The lines have to equal
tests/golden/op_pack_digests.json, recorded from the build as it was before it was split into packer and upload (the
recipe: profiles/INDEX_r24.md), whatever the number of build threads: the image does not depend on it."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pack_digest(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not available here")
    exe = tmp_path_factory.mktemp("pack_digest") / "pack_digest"
    csrc = os.path.join(ROOT, "stormruler_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    "-I" + csrc, os.path.join(ROOT, "tools", "sanitize", "pack_digest.cpp"), "-x", "c++",
                    os.path.join(csrc, "op_pack.hip"), "-o", str(exe), "-lpthread"], check=True)
    return str(exe)


def test_the_packed_operator_is_the_recorded_one_from_1_3_and_7_threads(pack_digest):
    with open(os.path.join(ROOT, "tests", "golden", "op_pack_digests.json")) as f:
        expected = json.load(f)
    assert len(expected) == 80
    for threads in ("1", "3", "7"):
        env = dict(os.environ, STORM_HIP_BUILD_THREADS=threads, STORM_HIP_BUILD_MIN_CHUNK="5")
        p = subprocess.run([pack_digest], env=env, capture_output=True, text=True, timeout=120, check=True)
        assert p.stdout.splitlines() == expected, f"{threads} threads"
