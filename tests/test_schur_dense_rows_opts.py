"""The schur_dense_rows option on the host: its library default and its path from pars.kkt to okkt_opts (no GPU needed)."""
import ctypes as C

from onephase_jl_amd import _lib as L
from onephase_jl_amd import kkt_system_solver as KS


def test_default_is_off():
    o = L.OkktOpts()
    assert L.load().okkt_default_opts(C.byref(o)) == L.OKKT_OK
    assert o.schur_dense_rows == 0


def test_pars_map_onto_okkt_opts():
    pars = KS.Class_parameters()
    assert pars.kkt.hip_schur_dense_rows == 0
    assert KS.okkt_opts_from_pars(pars.kkt) == {}                  # the defaults pass nothing
    pars.kkt.hip_schur_dense_rows = -1
    assert KS.okkt_opts_from_pars(pars.kkt) == {"schur_dense_rows": -1}
    pars.kkt.hip_schur_dense_rows = 200
    assert KS.okkt_opts_from_pars(pars.kkt) == {"schur_dense_rows": 200}
