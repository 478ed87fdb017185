"""Selected inversion without a GPU: the argument refusals of okkt_selinv and its exports on a NULL handle and on a host-symbolic-only
handle."""
import ctypes as C

import numpy as np

from onephase_jl_amd import _lib as L
from onephase_jl_amd import synth


def _host_handle():
    lib = L.load()
    o = L.OkktOpts()
    lib.okkt_default_opts(C.byref(o))
    o.host_symbolic_only = 1
    h = C.c_void_p()
    assert lib.okkt_create(C.byref(h), C.byref(o)) == L.OKKT_OK
    return lib, h


def test_null_handle_refused():
    lib = L.load()
    out = np.zeros(4)
    nnz = C.c_int64()
    info = L.OkktSelinvInfo()
    v, s = C.c_double(), C.c_int32()
    assert lib.okkt_selinv(None, C.byref(info)) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_diag(None, L.p_f64(out)) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_diag_dev(None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_on_pattern(None, L.p_f64(out), C.byref(nnz)) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_on_pattern_dev(None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_csc(None, None, None, None, C.byref(nnz)) == L.OKKT_ERR_INVALID
    assert lib.okkt_logdet(None, C.byref(v), C.byref(s)) == L.OKKT_ERR_INVALID


def test_host_symbolic_handle():
    lib, h = _host_handle()
    prob = synth.make_problem(300, 200, seed=1, well_scaled=True)
    K = synth.augmented_matrix(prob, delta=1e-8)
    dim = K.shape[0]
    cp, rv = L.i64(K.indptr), L.i64(K.indices)
    out = np.zeros(dim)
    nnz = C.c_int64()
    info = L.OkktSelinvInfo()
    v, s = C.c_double(), C.c_int32()
    # before the analysis: sizes are refused, the computation needs a device
    assert lib.okkt_get_inverse_csc(h, None, None, None, C.byref(nnz)) == L.OKKT_ERR_INVALID
    assert lib.okkt_get_inverse_on_pattern(h, None, C.byref(nnz)) == L.OKKT_ERR_INVALID
    assert lib.okkt_selinv(h, C.byref(info)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_analyze(h, dim, L.p_i64(cp), L.p_i64(rv), 0) == L.OKKT_OK
    # after it: the sizes come from the plan; everything that reads Z or D needs a device
    assert lib.okkt_get_inverse_csc(h, None, None, None, C.byref(nnz)) == L.OKKT_OK
    st = L.OkktStats()
    assert lib.okkt_get_stats(h, C.byref(st)) == L.OKKT_OK
    assert nnz.value == st.nnzL_stored
    assert lib.okkt_get_inverse_on_pattern(h, None, C.byref(nnz)) == L.OKKT_OK and nnz.value == K.nnz
    assert lib.okkt_get_inverse_on_pattern(h, None, None) == L.OKKT_ERR_INVALID
    assert lib.okkt_selinv(h, None) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_get_inverse_diag(h, L.p_f64(out)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_get_inverse_diag(h, None) == L.OKKT_ERR_INVALID
    zv = np.zeros(K.nnz)
    assert lib.okkt_get_inverse_on_pattern(h, L.p_f64(zv), C.byref(nnz)) == L.OKKT_ERR_NO_DEVICE
    colptr = np.zeros(dim + 1, dtype=np.int64)
    rowval = np.zeros(nnz.value, dtype=np.int64)
    val = np.zeros(nnz.value)
    assert lib.okkt_get_inverse_csc(h, L.p_i64(colptr), L.p_i64(rowval), L.p_f64(val), C.byref(nnz)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_logdet(h, C.byref(v), C.byref(s)) == L.OKKT_ERR_NO_DEVICE
    assert lib.okkt_logdet(h, None, C.byref(s)) == L.OKKT_ERR_INVALID
    assert b"host_symbolic_only" in lib.okkt_last_error(h)
    assert lib.okkt_destroy(h) == L.OKKT_OK
