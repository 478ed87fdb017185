"""The refusing paths of the C ABI layer (csrc/api*.cpp) as a table: every entry point of the layer called with a NULL handle, with a
host_symbolic_only handle analysed on a 3 x 3 pattern, and with the same handle in Schur mode, the integer arguments 1 or -1 and the
pointer arguments all NULL or all 64 zeroed doubles.  A host_symbolic_only handle is refused at the device gate, so no call reaches a
device and the table is the same with and without a GPU.  Each record is [handle case, function, ints, bufs, rc, okkt_last_error]: the
return code, the message and, through the fixed order of the calls on one handle, the calls that leave the previous message in place.

What the table pins is everything in front of the device gate and the gate itself.  A check that stands behind the gate is recorded as
the gate's answer (-2, "host_symbolic_only"): the "ld < ns" texts of the seven ld entries, and everything the Schur-mode and
refinement gates say after the device check ("no complete okkt_factor_schur", "... called before a factorisation", ...).  Those texts
are exercised by the GPU tests only (tests/test_gpu_schur_complement.py, test_gpu_schur_factor.py, test_gpu_schur_route.py, ...).

tests/golden/abi_refusals.json is collect() of the library before the layer was split into files (python tests/abi_refusals.py OUT
writes it); tests/test_abi_refusals.py compares."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from onephase_jl_amd import _lib as L  # noqa: E402

# the entry points of the ABI layer, without okkt_create, okkt_destroy, okkt_default_opts, okkt_version, okkt_last_error and
# okkt_debug_dataflow_queue
FUNCTIONS = [
    "okkt_set_early_exit", "okkt_set_perm", "okkt_analyze", "okkt_get_perm", "okkt_get_etree", "okkt_get_stats", "okkt_factor_dev",
    "okkt_factor", "okkt_solve_dev", "okkt_solve", "okkt_get_diag", "okkt_get_factor_csc", "okkt_dev_alloc", "okkt_dev_free",
    "okkt_dev_upload", "okkt_dev_download", "okkt_get_stream", "okkt_profile_dominant", "okkt_get_profile", "okkt_residual_dev",
    "okkt_residual", "okkt_solve_refine_dev", "okkt_solve_refine", "okkt_solve_gmres_dev", "okkt_schur_solve_gmres_dev",
    "okkt_solve_gmres", "okkt_schur_solve_gmres", "okkt_condest_dev", "okkt_schur_condest_dev", "okkt_condest", "okkt_schur_condest",
    "okkt_condest_indices", "okkt_forward_error_dev", "okkt_schur_forward_error_dev", "okkt_forward_error", "okkt_schur_forward_error",
    "okkt_set_scaling", "okkt_get_scaling_dev", "okkt_get_scaling", "okkt_set_schur", "okkt_factor_schur_dev", "okkt_factor_schur",
    "okkt_get_schur_dev", "okkt_get_schur", "okkt_schur_condense_dev", "okkt_schur_condense", "okkt_schur_expand_dev",
    "okkt_schur_expand", "okkt_schur_factor", "okkt_schur_factor_dev", "okkt_schur_get_factor", "okkt_schur_dense_solve",
    "okkt_schur_dense_solve_dev", "okkt_schur_solve", "okkt_schur_solve_dev", "okkt_schur_solve_refine_dev", "okkt_schur_solve_refine",
    "okkt_selinv", "okkt_get_inverse_diag_dev", "okkt_get_inverse_diag", "okkt_get_inverse_on_pattern_dev",
    "okkt_get_inverse_on_pattern", "okkt_get_inverse_csc", "okkt_logdet", "okkt_schur_get_inverse", "okkt_schur_get_inverse_dev",
    "okkt_schur_inverse_nonfinite", "okkt_schur_selinv", "okkt_schur_logdet", "okkt_pivot_report", "okkt_get_multipliers",
    "okkt_get_multipliers_dev", "okkt_get_rejected_pivots",
]
assert len(FUNCTIONS) == 73 and len(set(FUNCTIONS)) == 73

COLPTR = [0, 2, 4, 5]
ROWVAL = [0, 1, 1, 2, 2]
_INTS = (C.c_int, C.c_int32, C.c_int64)

# what the cross product misses: (function, handle case, {position of an integer argument after the handle: value})
GMRES = ["okkt_solve_gmres_dev", "okkt_schur_solve_gmres_dev", "okkt_solve_gmres", "okkt_schur_solve_gmres"]
REFINE = ["okkt_solve_refine_dev", "okkt_solve_refine", "okkt_schur_solve_refine_dev", "okkt_schur_solve_refine"]
LD = ["okkt_get_schur_dev", "okkt_get_schur", "okkt_schur_factor", "okkt_schur_factor_dev", "okkt_schur_get_factor",
      "okkt_schur_get_inverse", "okkt_schur_get_inverse_dev"]
NEEDS_ANALYSIS = ["okkt_get_perm", "okkt_get_etree", "okkt_get_stats", "okkt_get_factor_csc", "okkt_get_inverse_on_pattern",
                  "okkt_get_inverse_csc"]


def _create(lib, case):
    """A handle of the case: 'fresh' (no analysis), 'host' (analysed on the 3 x 3 pattern), 'schur' (the same with the Schur set {2})."""
    opts = L.OkktOpts()
    assert lib.okkt_default_opts(C.byref(opts)) == 0
    opts.host_symbolic_only = 1
    h = C.c_void_p()
    assert lib.okkt_create(C.byref(h), C.byref(opts)) == 0
    if case == "schur":
        idx = (C.c_int64 * 1)(2)
        assert lib.okkt_set_schur(h, 1, idx) == 0
    if case != "fresh":
        cp = (C.c_int64 * 4)(*COLPTR)
        rv = (C.c_int64 * 5)(*ROWVAL)
        assert lib.okkt_analyze(h, 3, cp, rv, 0) == 0
    return h


def _call(lib, h, name, ints, valid, keep):
    """name(h, ...): every integer argument ints (or its entry of the dict ints, 1 where it has none), every floating-point argument 0,
    every pointer NULL or 64 zeroed doubles of its own.  keep holds the buffers until the handle is destroyed."""
    res, argtypes = L.SIGNATURES[name]
    args = [h]
    for pos, t in enumerate(argtypes[1:]):
        if t in _INTS:
            args.append(ints.get(pos, 1) if isinstance(ints, dict) else ints)
        elif t is C.c_double:
            args.append(0.0)
        elif not valid:
            args.append(None)
        else:
            buf = (C.c_double * 64)()
            keep.append(buf)
            args.append(C.cast(buf, t))
    rc = getattr(lib, name)(*args)
    return int(rc) if rc is not None else 0      # (a NULL void* comes back as None)


def _int_pos(name, k):
    """Position (after the handle) of the k-th integer argument of name."""
    return [p for p, t in enumerate(L.SIGNATURES[name][1][1:]) if t in _INTS][k]


def collect():
    lib = L.load()
    assert not [f for f in FUNCTIONS if f in L.MISSING]
    out = []

    def run(case, name, combos):
        h = None if case == "null" else _create(lib, case)
        keep = []
        for label, ints, valid in combos:
            rc = _call(lib, h, name, ints, valid, keep)
            out.append([case, name, label, "valid" if valid else "null", rc, lib.okkt_last_error(h).decode()])
        if h is not None:
            assert lib.okkt_destroy(h) == 0

    for name in FUNCTIONS:
        run("null", name, [("1", 1, False), ("1", 1, True)])
    for case in ("host", "schur"):
        for name in FUNCTIONS:
            run(case, name, [("1", 1, False), ("1", 1, True), ("-1", -1, False), ("-1", -1, True)])
    for case in ("host", "schur"):
        for name in GMRES:       # integers: nrhs, restart, max_iters
            run(case, name, [("restart=65", {_int_pos(name, 1): 65}, True), ("max_iters=-1", {_int_pos(name, 2): -1}, True),
                             ("nrhs=-1,restart=65", {_int_pos(name, 0): -1, _int_pos(name, 1): 65}, True)])
        for name in REFINE:      # integers: nrhs, max_steps
            run(case, name, [("max_steps=-1", {_int_pos(name, 1): -1}, True), ("max_steps=-1", {_int_pos(name, 1): -1}, False)])
    for name in LD:              # the one integer: ld, below ns = 1
        run("schur", name, [("ld=0", {_int_pos(name, 0): 0}, True)])
    for name in NEEDS_ANALYSIS:
        run("fresh", name, [("1", 1, False), ("1", 1, True)])
    return out


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in collect()) + "\n]\n")      # one record per line
