"""Native artefact writer, host side (no GPU).

``ops.npy_header(n)`` must be byte for byte what ``np.save`` puts in front
of a 1-D float32 array of ``n`` elements: the file images the persister
builds are read back by ``np.load``, and ``tests/test_cycle_io.py``
compares whole files with ``np.save`` output.

The pool itself (``ops/hip/artefact_writer.*``, plain C++) runs in a
stand-alone program under ASAN+UBSAN and under TSAN, as
``tests/test_asan_host.py`` does for the philox header: nothing is loaded
into Python under a sanitizer.
"""
import io
import os
import subprocess

import numpy as np
import pytest
from numpy.lib import format as npy_format

from bodywork_mlops_demo_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"

HEADER_NS = sorted({0, 1, 9, 10, 99, 100}
                   | {10 ** k - 1 for k in range(1, 13)}
                   | {10 ** k for k in range(1, 13)})


def _numpy_header(n: int) -> bytes:
    # what np.save writes before the data; n elements are never allocated
    bio = io.BytesIO()
    npy_format.write_array_header_1_0(
        bio, {"descr": "<f4", "fortran_order": False, "shape": (n,)})
    return bio.getvalue()


def test_numpy_header_helper_is_np_save():
    for n in (0, 1, 9, 10, 1000):
        bio = io.BytesIO()
        np.save(bio, np.zeros(n, dtype=np.float32))
        raw = bio.getvalue()
        assert raw[:len(raw) - 4 * n] == _numpy_header(n)


@pytest.mark.parametrize("n", HEADER_NS)
def test_npy_header_equals_numpy(n):
    got = ops.npy_header(n)
    assert isinstance(got, bytes)
    assert got == _numpy_header(n)
    assert len(got) % 64 == 0


@pytest.mark.skipif(not os.path.exists(CLANGXX),
                    reason="ROCm clang++ not present")
@pytest.mark.timeout(300)
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_writer_pool_under_sanitizers(tmp_path, sanitizer):
    exe = str(tmp_path / "artefact_writer_host")
    build = subprocess.run(
        [CLANGXX, "-O1", "-std=c++17", "-g", "-pthread",
         f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all",
         os.path.join(REPO, "tests", "asan", "artefact_writer_host.cpp"),
         os.path.join(REPO, "bodywork_mlops_demo_amd", "ops", "hip",
                      "artefact_writer.cpp"),
         "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    run = subprocess.run([exe, str(out_dir)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.strip() == "ok"
    names = os.listdir(out_dir)
    assert not [f for f in names if f.startswith(".tmp-")]
    # 15 good jobs of the first pool + 6 drained by the second's destructor
    assert len(names) == 21
