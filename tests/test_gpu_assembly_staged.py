"""GPU tests of the staged big-front assembly (csrc/asm_pieces.h, k_big_assemble_staged in csrc/numeric.hip): flat piece records per
(front column, 512-row chunk) and index / value loads staged ahead of the LDS accumulation.  The contributions of a column are
applied in the order of the item lists on every assembly path, so the factor must equal, BIT FOR BIT, the one of the in-HBM path
(OKKT_ASM_CHUNKED=0 OKKT_ASM_LCOL=0: assemble_column<false, ...>, which reads ea_rec and never sees the records): D, the stored L,
the inertia and one solution; in Schur mode the assembled Schur front S as well.  Two settings are compared with it: the default
(every big front takes the staged kernel) and OKKT_ASM_CHUNK_MIN=2048 (only the fronts of more than 2048 rows take it, the others the
LDS-column kernel: the threshold the chunked kernel had).  The designs are listed in tests/assembly_staged_case.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["p2100", "p2049", "p2048", "p1025", "mid2150", "p2100-dup", "p2100-schur", "p2100-parted"]
SETTINGS = {"hbm": {"OKKT_ASM_CHUNKED": "0", "OKKT_ASM_LCOL": "0"}, "staged": {}, "staged-2048": {"OKKT_ASM_CHUNK_MIN": "2048"}}


def run(out, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("OKKT_ASM_")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "assembly_staged_case.py"), out] + CASES, cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "CASE_OK" in r.stdout, (env, r.stdout[-400:], r.stderr[-1500:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One process per setting of the switches, every case in it."""
    d = tmp_path_factory.mktemp("assembly_staged")
    return {name: run(str(d / f"{name}.npz"), env) for name, env in SETTINGS.items()}


@pytest.mark.parametrize("setting", ["staged", "staged-2048"])
@pytest.mark.parametrize("case", CASES)
def test_the_staged_assembly_equals_the_in_hbm_path_bit_for_bit(results, case, setting):
    a, b = results["hbm"], results[setting]
    n = int(a[f"{case}/n"])
    keys = sorted(k for k in a if k.startswith(case + "/"))
    assert keys == sorted(k for k in b if k.startswith(case + "/"))
    assert {f"{case}/d", f"{case}/x", f"{case}/inertia"} <= set(keys) and (f"{case}/Lx" in keys or f"{case}/S" in keys)
    assert np.isfinite(a[f"{case}/x"]).all() and a[f"{case}/x"].shape == (n,) and np.abs(a[f"{case}/x"]).max() > 0
    if f"{case}/Lx" in keys:
        assert a[f"{case}/Lx"].size > n and np.isfinite(a[f"{case}/Lx"]).all()
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
