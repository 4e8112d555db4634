"""CPU: the yardstick of cp_gauss_newton_dense (tests/gauss_newton_dense_reference.py) and everything the entry point answers before it touches a device.

Every listed case lies under the cap of 32 floors (the float64 restatement against the longdouble truth); with P = diag(w) the restatement is the diagonal
path's (tests/gauss_newton_reference.py ``contract``) to rounding; the drop rule; the workspace sizer; and every refusal, status and message, in the order
the header states, on fake non-null pointers nobody reads (tests/test_emulator_abi_errors_host.py: a call that came back late would launch on them)."""
import ctypes

import numpy as np
import pytest

import gauss_newton_dense_reference as gd
import gauss_newton_reference as gr
import jacobian_reference as jr

FAKE = 8      # a non-null pointer nobody reads


@pytest.mark.parametrize('case', gd.CASES, ids=gd.case_id)
def test_every_case_lies_under_the_cap(case):
    level = gd.worst_level(gd.draw(*case))
    print('%s: %.3g floors' % (gd.case_id(case), level))
    assert level <= gd.CAP


@pytest.mark.parametrize('case', [(9, 7, 17), (3, 32, 17), (33, 1, 65), (9, 7, 257)], ids=gd.case_id)
def test_a_diagonal_precision_is_the_diagonal_path(case):
    ops = gd.draw(*case)
    w = np.diagonal(ops['precision']).copy()
    w[::5] = 0.      # dropped columns as well
    dense = gd.contract(ops['J'], ops['value'], np.diag(w), ops['data'], 'f8')
    diagonal = gr.contract(ops['J'], ops['value'], w, ops['data'], 'f8')
    truth = gr.contract(ops['J'], ops['value'], w, ops['data'], jr.LD)
    # two summation orders of the same terms: each within the rule's allowance of the truth
    gr.assert_within(dense, truth, diagonal, 'dense restatement with a diagonal precision')
    assert gd.contract(ops['J'], ops['value'], np.diag(w), None, 'f8')[1:] == (None, None)


def test_drop_rule_of_the_restatement():
    ops = gd.draw(5, 3, 12)
    P, J, value, data = ops['precision'].copy(), ops['J'].copy(), ops['value'].copy(), ops['data'].copy()
    gone = np.array([0, 4, 5, 11])
    P[gone, gone] = 0.      # the diagonal alone: the rest of the rows and columns stays
    J[:, :, gone], value[:, gone[:2]], data[:, gone[2:]] = np.nan, np.inf, -np.inf
    kept = np.setdiff1d(np.arange(12), gone)
    for dtype in ('f8', jr.LD):
        masked = gd.contract(J, value, P, data, dtype)
        removed = gd.contract(ops['J'][:, :, kept], ops['value'][:, kept], ops['precision'][np.ix_(kept, kept)], ops['data'][:, kept], dtype)
        assert all(np.isfinite(m).all() and np.array_equal(m, r) for m, r in zip(masked, removed))      # added zeros change no bit


def sizer(lib, B, ndim, ncols):
    return int(lib.cp_gauss_newton_dense_workspace_doubles(B, ndim, ncols))


def test_workspace_sizer():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    for B, ndim, ncols in [(1, 1, 1), (9, 7, 17), (9, 7, 256), (9, 7, 257), (3, 32, 520), (10000, 8, 256), (0, 3, 5), (5, 3, 0)]:
        tiles = (ncols + 255) // 256
        assert sizer(lib, B, ndim, ncols) == ncols + tiles * B * (ndim * ndim + ndim + 1), (B, ndim, ncols)      # the mask, then the column tiles' partial sums
    for bad in [(-1, 3, 5), (4, 0, 5), (4, 3, -1)]:
        assert sizer(lib, *bad) == -_lib.CP_EINVAL and b'cp_gauss_newton_dense_workspace_doubles' in lib.cp_last_error()
    assert sizer(lib, 4, 33, 5) == -_lib.CP_EUNSUPPORTED and b'at most 32' in lib.cp_last_error()
    assert sizer(lib, 4, 3, (1 << 24) - 255) == -_lib.CP_EUNSUPPORTED and b'2^24 - 256 columns' in lib.cp_last_error()
    assert sizer(lib, 4, 3, (1 << 24) - 256) > 0
    assert sizer(lib, (1 << 31) * 16, 3, 5) == -_lib.CP_EUNSUPPORTED and b'row tiles of 16 points' in lib.cp_last_error()
    assert sizer(lib, 1 << 32, 32, 5) == -_lib.CP_EUNSUPPORTED      # one point per row tile


def entry(lib, B=4, ndim=3, ncols=5, ldj=5, ldv=5, ldd=5, ldp=5, jac=FAKE, value=FAKE, data=FAKE, precision=FAKE, fisher=FAKE, grad=FAKE, chi2=FAKE, work=FAKE,
          work_doubles=None):
    """(status, message) of cp_gauss_newton_dense on fake pointers (None: a null one); the workspace as the sizer asks unless given"""
    if work_doubles is None:
        work_doubles = max(sizer(lib, B, ndim, ncols), 0)
    p = lambda a: ctypes.c_void_p(a) if a else None      # noqa: E731
    status = lib.cp_gauss_newton_dense(p(jac), ldj, B, ndim, ncols, p(value), ldv, p(data), ldd, p(precision), ldp, p(fisher), p(grad), p(chi2), p(work), work_doubles, 0, None)
    return status, lib.cp_last_error().decode('utf-8') if status else ''


REFUSALS = [      # (what, arguments, status name, what the message holds); all of them before any device call
    ('B < 0', dict(B=-1), 'CP_EINVAL', '-1 points of 3 parameters over 5 columns'),
    ('ndim < 1', dict(ndim=0), 'CP_EINVAL', '4 points of 0 parameters'),
    ('ncols < 0', dict(ncols=-1, ldj=0, ldv=0, ldd=0, ldp=0), 'CP_EINVAL', 'over -1 columns'),
    ('ldj', dict(ldj=4), 'CP_EINVAL', 'row stride 4 of the Jacobian is less than its 5 columns'),
    ('ldv', dict(ldv=4), 'CP_EINVAL', 'row stride 4 of the value is less than its 5 columns'),
    ('ldd', dict(ldd=4), 'CP_EINVAL', 'row stride 4 of the data is neither 0 (one shared row) nor at least their 5 columns'),
    ('ldp', dict(ldp=4), 'CP_EINVAL', 'row stride 4 of the precision matrix is less than its 5 columns'),
    ('a stride before ndim > 32', dict(ndim=33, ldp=4), 'CP_EINVAL', 'precision matrix'),
    ('ndim > 32', dict(ndim=33), 'CP_EUNSUPPORTED', '33 parameters (at most 32)'),
    ('ndim > 32 before the null pointers', dict(ndim=33, jac=None), 'CP_EUNSUPPORTED', 'at most 32'),
    ('columns', dict(ncols=(1 << 24) - 255, ldj=1 << 24, ldv=1 << 24, ldd=0, ldp=1 << 24, work_doubles=0), 'CP_EUNSUPPORTED', '2^24 - 256 columns'),
    ('row tiles', dict(B=(1 << 31) * 16, work_doubles=0), 'CP_EUNSUPPORTED', 'at most 2^31 - 1 row tiles of 16 points'),
    ('the caps before the null pointers', dict(B=(1 << 31) * 16, fisher=None, work_doubles=0), 'CP_EUNSUPPORTED', 'row tiles'),
    ('null Jacobian', dict(jac=None), 'CP_EINVAL', 'cp_gauss_newton_dense: null pointer'),
    ('null value with data', dict(value=None), 'CP_EINVAL', 'null pointer'),
    ('null precision', dict(precision=None), 'CP_EINVAL', 'null pointer'),
    ('null fisher', dict(fisher=None), 'CP_EINVAL', 'null pointer'),
    ('null workspace', dict(work=None), 'CP_EINVAL', 'null pointer'),
    ('gradient without data', dict(data=None, chi2=None), 'CP_EINVAL', 'a gradient or chi2 is asked for without data'),
    ('chi2 without data', dict(data=None, grad=None), 'CP_EINVAL', 'a gradient or chi2 is asked for without data'),
    ('data without the gradient', dict(grad=None), 'CP_EINVAL', 'data is given: the gradient and chi2 are written'),
    ('data without chi2', dict(chi2=None), 'CP_EINVAL', 'data is given: the gradient and chi2 are written'),
    ('short workspace', dict(work_doubles=56), 'CP_EINVAL', 'workspace of 56 doubles, 57 needed (cp_gauss_newton_dense_workspace_doubles)'),
    ('ncols = 0: null fisher', dict(ncols=0, fisher=None), 'CP_EINVAL', 'null pointer'),
]


@pytest.mark.parametrize('what,kwargs,status,message', REFUSALS, ids=[refusal[0] for refusal in REFUSALS])
def test_refusals(what, kwargs, status, message):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    got, said = entry(lib, **kwargs)
    assert got == getattr(_lib, status) and message in said and said.startswith('cp_gauss_newton_dense: '), (got, said)


def test_nothing_to_do():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert entry(lib, B=0) == (_lib.CP_OK, '')
    assert entry(lib, B=0, jac=None, value=None, data=None, precision=None, fisher=None, grad=None, chi2=None, work=None) == (_lib.CP_OK, '')
    assert entry(lib, B=0, ndim=33)[0] == _lib.CP_EUNSUPPORTED and entry(lib, B=0, ldj=4)[0] == _lib.CP_EINVAL      # the checks come first


def test_python_front_has_the_keyword():
    import inspect
    from cosmoprimo_amd.emulators import tools
    for method in (tools.Emulator.gauss_newton, tools.Emulator.least_squares):
        assert inspect.signature(method).parameters['precision'].default is None      # without it a call is what it was
    assert list(inspect.signature(tools.gauss_newton_dense).parameters) == ['jacobian', 'value', 'precision', 'data']
    for engine in (tools.TaylorEmulatorEngine, tools.MLPEmulatorEngine):
        assert list(inspect.signature(engine.jacobian).parameters)[-1] == 'out'
