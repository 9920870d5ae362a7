"""CPU-side checks of the split arithmetic every matrix-core kernel rests on (multi-modal-gnn_amd/csrc/mma.h): the host
half of tests/split_cpu.hip, built with hipcc --cuda-host-only, runs the header's own macros and functions over random fp32
bit patterns.  The bounds are the ones the header states; no GPU is needed.

The scale rule of the f16 scatter (H2Scale / h2_decide_uniform) is run there too: its trajectories over random sequences of
block maxima must be those of the numpy restatement tests/h2_ref.py, and a host simulation of one column of a wave (the
header's rule and split8_h2, fp32 accumulation, one item per block) must meet the two bars that
tests/test_scatter_scale_gpu.py holds the kernel to, on the same named profiles and on random walks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import h2_ref as H

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
    rep = {"h2walk": []}
    for line in out.splitlines():
        name, *fields = line.split()
        if name == "h2walk":            # one walk: "bits:inf:e:path" per block, then "out:e_out"
            rep["h2walk"].append(([tuple(int(v, 16 if i == 0 else 10) for i, v in enumerate(f.split(":"))) for f in fields[:-1]],
                                  int(fields[-1].split(":")[1])))
            continue
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


# ------------------------------------------------------------------------------------------ the wave's scale rule
def test_scale_rule_follows_the_numpy_restatement(report):
    """Random walks of the block maximum's exponent (steps up to +-150 / 12 / 3), all-zero blocks and infinities strewn in:
    the header's rule and tests/h2_ref.py give the same e and the same path at every block, and the same final e."""
    walks = report["h2walk"]
    assert len(walks) >= 600
    seen = np.zeros(5, np.int64)
    for blocks, e_out in walks:
        m = np.array([b[0] for b in blocks], dtype=np.uint32).view(np.float32)
        es, paths, eo = H.walk(m, has_inf=[b[1] for b in blocks])
        assert es.tolist() == [b[2] for b in blocks], (m, [b[1] for b in blocks])
        assert paths.tolist() == [b[3] for b in blocks], (m, [b[1] for b in blocks])
        assert eo == e_out
        seen += np.bincount(paths, minlength=5)
    assert (seen >= 50).all(), seen       # every outcome of the rule many times: nothing, first, lower, outlier, re-anchor


IN_WINDOW = {"flat": "first", "rise9": "lower", "fall14": "first", "step12": "outlier", "step30": "outlier",
             "spike": "outlier", "step95": "reanchor", "zero_head": "first", "cols14": "first"}
BELOW_WINDOW = {"fall23": "first", "fall46": "first", "cols20": "first", "step140": "reanchor"}


@pytest.mark.parametrize("name", list(IN_WINDOW) + list(BELOW_WINDOW))
def test_simulated_wave_meets_the_bars_on_the_named_profiles(report, name):
    """One column of a 24-block wave, item b = the 16 values of block b.  In-window profiles: every item within 6e-7 of its own
    sum of |terms|, finite, exactly 0 where that sum is 0.  Below-window profiles: within 6e-7 mag + 16 * 2^-25 * 2^-e, e from
    the rule (tests/h2_ref.floor_exponents).  Every wave took the path the profile is named for."""
    r = report["h2sim_" + name]
    path = IN_WINDOW.get(name) or BELOW_WINDOW[name]
    assert r["waves"] >= 2000 and r["items"] == 24 * r["waves"]
    assert r["w_first"] == r["waves"] and r["w_" + path] == r["waves"]
    assert r["bad_floor"] == 0
    if name in IN_WINDOW:
        assert r["in_window"] == r["items"] and r["bad_in"] == 0 and r["worst_all"] <= 6e-7
    else:
        assert r["in_window"] == 0 and r["worst_all"] > 6e-7       # (the profile does leave the window: the first bar alone fails)


def test_simulated_wave_meets_the_bars_on_random_walks(report):
    r = report["h2sim_walks"]
    assert r["walks_in_window"] >= 1e5 and r["items"] == 24 * r["walks"]
    assert r["bad_in"] == 0 and r["worst_in"] <= 6e-7 and r["bad_floor"] == 0
    assert min(r["first"], r["lower"], r["outlier"], r["reanchor"]) >= 1000
