"""CPU-side checks of the split arithmetic every matrix-core kernel rests on (multi-modal-gnn_amd/csrc/mma.h): the host
half of tests/split_cpu.hip, built with hipcc --cuda-host-only, runs the header's own macros and functions over random fp32
bit patterns.  The bounds are the ones the header states; no GPU is needed."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find_hipcc():
    for c in ("hipcc", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")):
        if shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """{check name: {key: number}} as printed by the program."""
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc found (PATH, $ROCM_PATH/bin, /opt/rocm/bin): the split program cannot be built")
    exe = tmp_path_factory.mktemp("split_cpu") / "split_cpu"
    subprocess.run([hipcc, "-O2", "-std=c++17", "--cuda-host-only", "--offload-arch=gfx950",
                    os.path.join(REPO, "tests", "split_cpu.hip"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    rep = {}
    for line in out.splitlines():
        name, *fields = line.split()
        rep[name] = {k: float(v) for k, v in (f.split("=") for f in fields)}
    return rep


def test_three_bf16_pieces_add_up_exactly(report):
    r = report["split3"]
    assert r["n"] >= 1e6 and r["failures"] == 0
    assert report["split8"]["n"] >= 1e6 and report["split8"]["failures"] == 0      # mmg_split8 = eight MMG_SPLIT3


def test_truncation_pieces_are_bf16_and_add_up_exactly(report):
    r = report["trunc"]
    assert r["n"] >= 1e6 and r["low_bits_set"] == 0 and r["sum_failures"] == 0


def test_two_f16_pieces_keep_22_bits(report):
    r = report["h2"]
    assert r["n"] >= 2e6 and r["bound"] == 2.0 ** -22
    assert r["failures"] == 0 and r["worst"] <= 2.0 ** -22


def test_pow2_is_ldexp(report):
    assert report["pow2"] == {"n": 254, "failures": 0}


def test_c_layout_rows_are_a_bijection(report):
    assert report["c_row"] == {"rows_hit_once": 32, "outside": 0}


def test_both_product_orders_are_fp32_grade_and_differ(report):
    r = report["x6"]
    assert r["n"] >= 5e5 and r["alo_failures"] == 0 and r["blo_failures"] == 0
    assert max(r["worst_alo"], r["worst_blo"]) <= 3 * 2.0 ** -24
    assert r["differ"] > 0          # the term order reaches the last bit: it is part of each kernel's contract
