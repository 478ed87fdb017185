"""GPU tests: the KKT layer's assembly and row kernels (csrc/kkt.hip) against exact arithmetic on designed inputs (tests/kkt_designs.py):
Q of the Schur kinds on every route of the assembly (G = 16, 8, 4 of k_assemble_schur_lds and the contribution lists of
k_assemble_schur, OKKT_SCHUR_GROUPS), the bordered system, the symmetric kind's K, System_rhs, dy / ds of the Schur kinds and the
N err, every lane count of the segmented products -- each value within the rounding bound of its exact value (tests/kkt_exact.py),
the route variants bitwise equal.  Duplicated entries are refused by the C ABI and summed by the Python binding, for every kind."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import kkt_designs as KD
import kkt_exact as KE
from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(KD.DESIGNS)
FACTORED = [n for n, d in KD.DESIGNS.items() if d.factor]
BORDER = [n for n, d in KD.DESIGNS.items() if d.dense]
# the schur_direct N err whose current iterate differs from the factor iterate, peaking in the last row of the last, partial workgroup
PEAK = "special:schur_direct:b32:1.0:0"
NAN_GRAD = "special:schur:b8:0:1"
ETA = (0.5, 0.25, 0.375)


def _case(tmp_path_factory, env, mode, names):
    out = str(tmp_path_factory.mktemp("kkt_case") / "case.npz")
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kkt_assembly_case.py"), out, mode] + names, cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "CASE_OK" in r.stdout, (env, r.stdout[-400:], r.stderr[-2000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return _case(tmp_path_factory, {}, "full", ALL + [PEAK, NAN_GRAD])


@pytest.fixture(scope="module")
def capped(tmp_path_factory):
    return {g: _case(tmp_path_factory, {"OKKT_SCHUR_GROUPS": str(g)}, "q", ALL) for g in (8, 4, 0)}


@pytest.fixture(scope="module")
def dense_dot_off(tmp_path_factory):
    return _case(tmp_path_factory, {"OKKT_DENSE_DOT": "0"}, "full", BORDER)


def mat(res, tag):
    p = res[f"{tag}/Ap"]
    return sp.csc_matrix((res[f"{tag}/Ax"], res[f"{tag}/Ai"], p), shape=(len(p) - 1, len(p) - 1))


def current(d, tag):
    """The current iterate run() of kkt_assembly_case used for tag: (J, s, y, grad, cons, mu, pen)."""
    last = float(tag.split(":")[3]) if tag.startswith("special:") else 0.0
    J2, s2, y2 = KD.moved(d, last=last)
    p = KD.point(d)
    grad = p["grad"].copy()
    if tag.startswith("special:") and tag.endswith(":1"):
        grad[len(grad) // 2] = np.nan
    return J2, s2, y2, grad, p["cons"], p["mu"], 1e-4


assert_within = KE.assert_within


# ---- 1. Q of the Schur kinds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_schur_matrix_pattern_and_bound(full, name):
    d = KD.DESIGNS[name]
    n = d.n
    tag = f"{name}/schur"
    A = mat(full, tag)
    drows = KD.dense_rows(d.J, d.dense)
    assert np.array_equal(full[f"{tag}/drows"], drows)
    kd = len(drows)
    # the pattern: tril(|J_s|'|J_s| + |H| + I), then per column the border rows n + r of the dense rows holding it; n + r: its diagonal
    P, _ = KD.q_pattern(d.H, d.J, drows)
    Jd = d.J.tocsr()[drows].tocsc()
    for j in range(n):
        want = list(P.indices[P.indptr[j]:P.indptr[j + 1]]) + [n + r for r in Jd.indices[Jd.indptr[j]:Jd.indptr[j + 1]]]
        assert list(A.indices[A.indptr[j]:A.indptr[j + 1]]) == want, (name, j)
    for r in range(kd):
        assert list(A.indices[A.indptr[n + r]:A.indptr[n + r + 1]]) == [n + r]
    sig = d.y / d.s
    if name == "long_row":
        r = KE.q_ratios_single_term(A, d.H, d.J, sig)
    else:
        r = KE.q_ratios(A, KE.q_exact(d.H, d.J, sig, drows), n)
    assert_within(r, name)
    # the same matrix from schur_direct, and from a second form_system of either kind, bit for bit
    assert np.array_equal(full[f"{name}/schur_direct/Ax"], A.data)
    if f"{tag}/Ax2" in full:
        assert np.array_equal(full[f"{tag}/Ax2"], A.data)
        assert np.array_equal(full[f"{name}/schur_direct/Ax2"], A.data)
    if kd == 0:      # schur_diag = diag(Q) (schur.jl:56)
        assert np.array_equal(full[f"{tag}/sd"], A.diagonal()[:n])


@pytest.mark.parametrize("G", [8, 4, 0])
@pytest.mark.parametrize("name", ALL)
def test_schur_routes_are_bitwise_equal(full, capped, name, G):
    """OKKT_SCHUR_GROUPS caps G: every design is assembled by every route its longest column allows -- the same bits."""
    c = capped[G]
    tag = f"{name}/schur"
    for part in ("Ap", "Ai", "Ax"):
        assert np.array_equal(c[f"{tag}/{part}"], full[f"{tag}/{part}"]), (name, G, part)


# ---- 2. the bordered system ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BORDER)
def test_border_is_bitwise_and_schur_diag_within_bound(full, name):
    d = KD.DESIGNS[name]
    n = d.n
    drows = KD.dense_rows(d.J, d.dense)
    assert len(drows) == d.expect["kd"]
    for kind in ("schur", "schur_direct"):
        A = mat(full, f"{name}/{kind}").toarray()
        assert np.array_equal(A[n:, :n], d.J.tocsr()[drows].toarray())
        assert np.array_equal(np.diag(A[n:, n:]), -(d.s[drows] / d.y[drows]))
        assert np.count_nonzero(A[n:, n:] - np.diag(np.diag(A[n:, n:]))) == 0
        assert_within(KE.diag_ratios(full[f"{name}/{kind}/sd"], d.H, d.J, d.y / d.s), (name, kind))


# ---- 3. the symmetric kind's K -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_symmetric_matrix_copies_the_inputs(full, name):
    d = KD.DESIGNS[name]
    n, m = d.n, d.m
    K = mat(full, f"{name}/symmetric")
    assert K.shape == (n + m, n + m)
    H, J = d.H.tocsc(), d.J.tocsc()
    for j in range(n):
        rows = list(K.indices[K.indptr[j]:K.indptr[j + 1]])
        vals = K.data[K.indptr[j]:K.indptr[j + 1]]
        hr = list(H.indices[H.indptr[j]:H.indptr[j + 1]])
        hv = H.data[H.indptr[j]:H.indptr[j + 1]]
        jr = [n + i for i in J.indices[J.indptr[j]:J.indptr[j + 1]]]
        lead = [] if (hr and hr[0] == j) else [j]          # a missing diagonal is stored, as an explicit 0
        assert rows == lead + hr + jr, (name, j)
        assert np.array_equal(vals, np.concatenate([np.zeros(len(lead)), hv, J.data[J.indptr[j]:J.indptr[j + 1]]])), (name, j)
    assert np.array_equal(K.indptr[n:] - K.indptr[n], np.arange(m + 1))
    assert np.array_equal(K.indices[K.indptr[n]:], np.arange(n, n + m))
    assert np.array_equal(K.data[K.indptr[n]:], -(d.s / d.y))
    assert_within(KE.diag_ratios(full[f"{name}/symmetric/sd"], d.H, d.J, d.y / d.s), name)


# ---- 4. System_rhs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FACTORED)
def test_system_rhs_exact(full, name):
    d = KD.DESIGNS[name]
    J2, s2, y2, grad, cons, mu, pen = current(d, name)
    for kind in ("schur", "schur_direct", "symmetric", "clever_symmetric"):
        t = f"{name}/{kind}"
        for r, what in zip(KE.rhs_ratios(J2, grad, cons, s2, y2, mu, pen, ETA, full[f"{t}/rD"], full[f"{t}/rP"], full[f"{t}/rC"]),
                           ("dual_r", "primal_r", "comp_r")):
            assert_within(r, (name, kind, what))


# ---- 5. dy, ds of the Schur kinds --------------------------------------------------------------------------------------------------
def _check_dyds(res, d, tag, kind):
    J2, s2, y2 = current(d, tag)[:3]
    direct = kind == "schur_direct"
    J, y, s = (J2, y2, s2) if direct else (d.J, d.y, d.s)
    rdy, rds = KE.dyds_ratios(J, res[f"{tag}/dx"], res[f"{tag}/rP"], res[f"{tag}/rC"], y, s, res[f"{tag}/dy"], res[f"{tag}/ds"], direct)
    assert_within(rdy, (tag, "dy"))
    assert_within(rds, (tag, "ds"))


@pytest.mark.parametrize("kind", ["schur", "schur_direct"])
@pytest.mark.parametrize("name", FACTORED)
def test_schur_dy_ds_exact(full, name, kind):
    _check_dyds(full, KD.DESIGNS[name], f"{name}/{kind}", kind)


# ---- 6. N err ---------------------------------------------------------------------------------------------------------------------------
def _check_err(res, d, tag):
    return KE.check_err(res, d, tag, KD.shift(d))


@pytest.mark.parametrize("kind", ["schur", "schur_direct", "symmetric", "clever_symmetric"])
@pytest.mark.parametrize("name", FACTORED)
def test_kkt_error_exact(full, name, kind):
    _check_err(full, KD.DESIGNS[name], f"{name}/{kind}")


def test_kkt_error_peak_in_the_last_row_of_a_partial_workgroup(full):
    """The direct kind at a current iterate that is not the factor iterate: a genuinely large N err (its dy, ds come from the current
    iterate, the error from the factor iterate), whose maxima sit in the last row of the last, partial workgroup of k_err_dual and
    k_err_pc -- a launch that lost that workgroup would report the runner-up instead, far outside the bound."""
    d = KD.DESIGNS[PEAK.split(":")[2]]
    r = KD.routes(d)
    assert d.n % (256 // r["lprJc"]) and d.m % (256 // r["lprJr"])
    for (e, b), last in zip(_check_err(full, d, PEAK), (d.n - 1, d.m - 1, d.m - 1)):
        e = np.array([float(v) for v in e])
        assert int(np.argmax(e)) == last
        assert e[last] - b[last] > np.max(np.delete(e + b, last)) and e[last] > 1e-6
    _check_dyds(full, d, PEAK, "schur_direct")


def test_nan_in_grad_gives_nan_norms(full):
    err = full[f"{NAN_GRAD}/err"]
    assert np.isnan(err[0]) and np.isnan(err[3]) and np.isnan(err[4]) and np.isnan(err[5])
    assert np.isnan(full[f"{NAN_GRAD}/rD"]).any()


@pytest.mark.parametrize("name", BORDER)
def test_dense_dot_off(dense_dot_off, full, name):
    """OKKT_DENSE_DOT=0: the row kernels walk the dense rows themselves -- the same bounds."""
    d = KD.DESIGNS[name]
    for kind in ("schur", "schur_direct"):
        tag = f"{name}/{kind}"
        assert np.array_equal(dense_dot_off[f"{tag}/Ax"], full[f"{tag}/Ax"])
        _check_dyds(dense_dot_off, d, tag, kind)
        _check_err(dense_dot_off, d, tag)


# ---- 7. duplicated entries ------------------------------------------------------------------------------------------------------
def _with_duplicates(A, k):
    """A as a non-canonical CSC: the first k stored entries split into two halves (exact), rows of column 0 reversed."""
    A = A.tocsc()
    rows, vals, ptr = [], [], [0]
    done = 0
    for j in range(A.shape[1]):
        r, v = list(A.indices[A.indptr[j]:A.indptr[j + 1]]), list(A.data[A.indptr[j]:A.indptr[j + 1]])
        rr, vv = [], []
        for a, x in zip(r, v):
            if done < k:
                rr += [a, a]; vv += [x / 2, x / 2]; done += 1
            else:
                rr.append(a); vv.append(x)
        rows += rr; vals += vv; ptr.append(len(rows))
    out = sp.csc_matrix((np.array(vals), np.array(rows), np.array(ptr)), shape=A.shape)
    assert not out.has_canonical_format
    return out


def test_duplicate_entries_are_refused_by_the_abi():
    lib = L.load()
    d = KD.DESIGNS["tiny8"]
    for which in ("J", "H"):
        for kind in (L.OKKT_KKT_SCHUR, L.OKKT_KKT_SCHUR_DIRECT, L.OKKT_KKT_SYMMETRIC, L.OKKT_KKT_CLEVER_SYMMETRIC):
            H = _with_duplicates(d.H, 3) if which == "H" else d.H.tocsc()
            J = _with_duplicates(d.J, 3) if which == "J" else d.J.tocsc()
            k = C.c_void_p()
            o = L.OkktOpts()
            lib.okkt_default_opts(C.byref(o))
            assert lib.okkt_kkt_create(C.byref(k), C.byref(o), kind) == L.OKKT_OK
            Hp, Hi, Jp, Ji = (L.i64(a) for a in (H.indptr, H.indices, J.indptr, J.indices))
            rc = lib.okkt_kkt_set_structure(k, d.n, d.m, L.p_i64(Hp), L.p_i64(Hi), L.p_i64(Jp), L.p_i64(Ji), 0)
            msg = lib.okkt_kkt_last_error(k).decode()
            lib.okkt_kkt_destroy(k)
            assert rc == L.OKKT_ERR_INVALID, (which, kind, rc)
            assert msg.startswith(f"{which}: column ") and "after row" in msg and "strictly increasing" in msg, msg


def test_duplicate_entries_are_summed_by_the_binding_for_every_kind():
    """The binding canonicalises (sum_duplicates, as sparse() does): the same bits as the canonical input, in all four kinds, and the
    four kinds agree on the direction."""
    d = KD.DESIGNS["tiny8"]
    p = KD.point(d)
    dirs = {}
    for kind in ("schur", "schur_direct", "symmetric", "clever_symmetric"):
        got = []
        for H, J in ((d.H, d.J), (_with_duplicates(d.H, 4), _with_duplicates(d.J, 5))):
            it = KS.Class_iterate(x=p["x"], y=d.y, s=d.s, mu=p["mu"], J=J, H=H, grad=p["grad"], cons=p["cons"])
            k = KS.HIP_KKT_solver(kind)
            k.initialize_b(it)
            k.form_system_b(it)
            A = k.matrix()
            assert k.factor_b(KD.shift(d)) in (0, 1)
            k.kkt_associate_rhs_b(it, KS.Reduct_stable())
            k.compute_direction_b()
            got.append((A, k.dir.x.copy(), k.dir.y.copy(), k.dir.s.copy()))
            k.finalize_b()
        (A0, *v0), (A1, *v1) = got
        assert np.array_equal(A0.indptr, A1.indptr) and np.array_equal(A0.indices, A1.indices) and np.array_equal(A0.data, A1.data), kind
        for a, b in zip(v0, v1):
            assert np.array_equal(a, b), kind
        dirs[kind] = v0
    for kind, v in dirs.items():
        for a, b in zip(v, dirs["symmetric"]):
            assert np.max(np.abs(a - b)) <= 1e-8 * max(1.0, np.max(np.abs(b))), kind
