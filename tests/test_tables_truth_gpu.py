"""GPU: the two (k, z) table-row kernels of csrc/cp_spline.hip -- tables_rows_kernel (cp_tables_rows) and tables_rows_direct_kernel
(cp_tables_rows_direct) -- through their C entry points against the longdouble truth of tests/tables_truth.py, at their launch, tile, seam and route edges.
tests/test_tables_truth_host.py holds the truth to scipy, every case used here to the cap of its level and every exponent case to the side of
300 / 308.25 / -323.3 it claims.

Allowance: ALLOW = 16 levels of the float64 restatement per table (a block is one table's output, distances against the table's largest |argument|, the
level floored at 1.1e-16 and taken on the ARGUMENT of the epilogue); roots held squared + 3 FLOOR of the value; 10^x: ln 10 times the argument's allowance
+ 4e-15 relative, + 2 units of 2^-1074 where the result is subnormal, 0 and Inf exactly where 10^x leaves the doubles.

Every call writes into a buffer of canaries (64 in front, 64 rows of nq + 64 behind): every element written, none outside.  The tables, the second derivatives
and the (y, M) pairs are followed by 64 rows of NaN the kernels must never bring into a result, and are compared with what was uploaded after every call.
Every call is made twice on fresh buffers and gives the same bits; every call of the direct kernel is made with two arrays and with (y, M) pairs (d_m
null) and gives the same bits.  The direct kernel is handed the second derivatives the library computes (SplineRows.second_derivatives).  Each test
prints the largest fraction of its allowance (MEASURED lines: per kernel)."""
import numpy as np
import pytest

import tables_truth as tt
from sigma_device import CANARY, synchronized

pytestmark = pytest.mark.gpu

WORST = {}
PLANS = {}
KERNELS = ('rows', 'direct')


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


def note(kernel, group, fraction):
    WORST[kernel, group] = max(WORST.get((kernel, group), 0.), fraction)
    print('MEASURED %-6s %-10s largest fraction of the allowance so far %.3f' % (kernel, group, WORST[kernel, group]))
    return fraction


def plans(env, c, zq=None):
    """The z operator, both k plans and the plan of the second derivatives of a case (built once)."""
    from cosmoprimo_amd.spline import LinearOperator, SplineRows, dense_operator
    key = (id(c), None if zq is None else len(zq))
    if key not in PLANS:
        dev = env[3]
        x, xq = c['x'], c['xq']
        opz = LinearOperator.dense(dense_operator(c['zk'], c['zq'] if zq is None else zq, bc=c['zbc'], extrapolate=c['extrapolate']), device=dev)
        PLANS[key] = dict(c=c, opz=opz)
        if not c.get('direct_only'):
            PLANS[key]['opx'] = LinearOperator.spline(x, xq, bc=tt.K_BC, extrapolate=False, device=dev)
        if x.size == 4:      # one cubic through four knots: the rows kernels of the second derivatives refuse it, the direct kernel has no plan to take
            with pytest.raises(NotImplementedError):
                SplineRows(x, xq, bc=tt.K_BC, extrapolate=False, device=dev)
        else:
            PLANS[key].update(kplan=SplineRows(x, xq, bc=tt.K_BC, extrapolate=False, device=dev), mplan=SplineRows(x, x[[0, -1]], bc=tt.K_BC, device=dev))
    return PLANS[key]


def guarded_input(env, flat, n):
    """The array followed by 64 rows of n NaN (x 2 for pairs: the caller's n)."""
    torch, dev = env[0], env[3]
    buf = torch.full((flat.numel() + 64 * n,), float('nan'), dtype=torch.float64, device=dev)
    buf[:flat.numel()] = flat.reshape(-1)
    return buf


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype='f8'), np.ascontiguousarray(b, dtype='f8')
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def call(env, kernel, P, t, nb, post, scale, layout='two', nzq=None):
    """One call on fresh buffers: (nb, nzq, nq)."""
    torch, _lib, lib, dev, stream = env
    c = P['c']
    _, nzin, n, cnzq, nq = c['shape']
    nzq = cnzq if nzq is None else nzq
    tin = guarded_input(env, torch.as_tensor(np.array(t[:nb], dtype='f8'), device=dev), n)
    inputs = [tin]
    if kernel == 'direct':
        tv = tin[:nb * nzin * n].view(nb, nzin, n)
        clean = torch.as_tensor(np.array(np.where(np.isnan(t[:nb]), c['t'][:nb], t[:nb])), device=dev)      # (a NaN entry is put into y alone: the M of the clean table)
        if layout == 'pairs':
            ym = P['mplan'].second_derivatives(clean, pairs=True)
            ym[..., 0] = tv
            inputs = [guarded_input(env, ym, 2 * n)]
            pointers = (inputs[0].data_ptr(), None)
        else:
            inputs.append(guarded_input(env, P['mplan'].second_derivatives(clean), n))
            pointers = (tin.data_ptr(), inputs[1].data_ptr())
    before = [synchronized(torch, a).copy() for a in inputs]
    count = nb * nzq * nq
    out = torch.full((64 + count + 64 * nq + 64,), CANARY, dtype=torch.float64, device=dev)
    ptr = out.data_ptr() + 64 * 8
    if kernel == 'rows':
        assert lib.cp_tables_rows_available(P['opx']._handle, P['opz']._handle) == 1
        status = lib.cp_tables_rows(P['opx']._handle, P['opz']._handle, tin.data_ptr(), ptr, nb, tt.POST[post], float(scale), stream)
    else:
        status = lib.cp_tables_rows_direct(P['kplan']._handle, P['opz']._handle, pointers[0], pointers[1], ptr, nb, tt.POST[post], float(scale), stream)
    _lib.check(status)
    host = synchronized(torch, out)
    assert (host[:64] == CANARY).all(), 'elements in front of the output were written'
    assert (host[64 + count:] == CANARY).all(), '{:d} elements behind the output were written'.format(int((host[64 + count:] != CANARY).sum()))
    body = host[64:64 + count]
    assert not (body == CANARY).any(), '{:d} output elements were not written'.format(int((body == CANARY).sum()))
    for a, b in zip(inputs, before):
        assert same_bits(synchronized(torch, a), b), 'an input was changed'
    return body.reshape(nb, nzq, nq)


def run(env, c, post, group, kernels=KERNELS, nb=None, t=None, judge=True, P=None):
    """Both kernels: twice on fresh buffers, the direct kernel in both layouts, the same bits; judged against the case.  {kernel: (nb, nzq, nq)}."""
    P = plans(env, c) if P is None else P
    nb = c['shape'][0] if nb is None else nb
    t = c['t'] if t is None else t
    got = {}
    for kernel in kernels:
        if kernel == 'direct' and 'kplan' not in P:
            continue
        first = call(env, kernel, P, t, nb, post, c['scale'])
        assert same_bits(call(env, kernel, P, t, nb, post, c['scale']), first), '%s: two calls, other bits' % kernel
        if kernel == 'direct':
            assert same_bits(call(env, kernel, P, t, nb, post, c['scale'], layout='pairs'), first), '(y, M) pairs and two arrays: other bits'
        if judge:
            what = '%s %s, post %s, scale %g, %d tables' % (kernel, c['shape'][1:], post, c['scale'], nb)
            assert note(kernel, group, tt.fraction(first, c, post, what)) <= 1., what
        got[kernel] = first
    return got


# ---- wavenumbers, redshifts, knots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nq', tt.NQ)
def test_wavenumbers(env, nq):
    """The direct kernel's wave tiles of 16, its four steps of 64 and its workgroup tile of 256; cp_tables_rows' waves of 64 and windows."""
    c = tt.case(nq=nq)
    for post in (None, 'exp10'):
        run(env, c, post, 'nq')


@pytest.mark.parametrize('nq', tt.NZQ_NQ)
@pytest.mark.parametrize('nzq', tt.NZQ)
def test_redshifts(env, nzq, nq):
    """Both sides of nzq = 64 (``full``), end cubics continued; and NaN rows for a plan built without extrapolation."""
    for zq in ('beyond', 'nan_z'):
        c = tt.case(nzq=nzq, nq=nq, zq=zq)
        if zq == 'nan_z' and nzq >= 3:
            assert np.isnan(c['truth'][:, 0]).all() and np.isnan(c['truth'][:, -1]).all() and not np.isnan(c['truth'][:, 1]).any()
        for post in (None, 'exp10'):
            run(env, c, post, 'nzq')


@pytest.mark.parametrize('nzin', tt.NZIN)
def test_input_redshifts(env, nzin):
    """Both sides of nz_pad = 16 / 32: the rows past the table repeat its last one (the NaN rows behind the tables never reach a result)."""
    c = tt.case(nzin=nzin, nzq=64, nq=80, zq='inside')
    for post in (None, 'exp10'):
        run(env, c, post, 'nzin')
    run(env, tt.case(nzin=nzin), None, 'nzin')


@pytest.mark.parametrize('n', tt.N_KNOTS)
def test_knots(env, n):
    """cp_tables_rows' chunks of 16 knots and the partial last one; wavenumbers outside the knots: NaN columns, first and last of a row."""
    for kq in ('inside', 'outside'):
        c = tt.case(n=n, kq=kq)
        if kq == 'outside':
            assert np.isnan(c['truth'][..., :2]).all() and np.isnan(c['truth'][..., -2:]).all() and not np.isnan(c['truth'][..., 2:-2]).any()
        for post in (None, 'exp10'):
            run(env, c, post, 'n')


def test_refusals(env):
    """33 input or 65 output redshifts: CP_EUNSUPPORTED by both entry points; a k plan that does not span the knots: by the direct kernel."""
    torch, _lib, lib, dev, stream = env
    from cosmoprimo_amd.spline import LinearOperator, SplineRows
    c = tt.case()
    P = plans(env, c)
    rng = np.random.default_rng(0)
    t = torch.zeros((3 * 33 * 40 * 2,), dtype=torch.float64, device=dev)
    out = torch.full((3 * 65 * 70 + 1,), CANARY, dtype=torch.float64, device=dev)
    for shape in ((7, 33), (65, 5)):
        wide = LinearOperator.dense(rng.normal(size=shape), device=dev)
        assert lib.cp_tables_rows_available(P['opx']._handle, wide._handle) == 0
        assert lib.cp_tables_rows(P['opx']._handle, wide._handle, t.data_ptr(), out.data_ptr(), 3, 0, 1., stream) == _lib.CP_EUNSUPPORTED
        assert lib.cp_tables_rows_direct(P['kplan']._handle, wide._handle, t.data_ptr(), t.data_ptr(), out.data_ptr(), 3, 0, 1., stream) == _lib.CP_EUNSUPPORTED
        assert lib.cp_tables_rows_direct(P['kplan']._handle, wide._handle, t.data_ptr(), None, out.data_ptr(), 3, 0, 1., stream) == _lib.CP_EUNSUPPORTED
    x = tt.st.knots('geom1.05', 504)
    half = SplineRows(x, tt.k_queries(x, 70, 'half'), bc=tt.K_BC, device=dev)
    assert half.window[:2] != (0, 504)
    t = torch.zeros((3 * 5 * 504,), dtype=torch.float64, device=dev)
    assert lib.cp_tables_rows_direct(half._handle, P['opz']._handle, t.data_ptr(), t.data_ptr(), out.data_ptr(), 3, 0, 1., stream) == _lib.CP_EUNSUPPORTED
    assert (synchronized(torch, out) == CANARY).all()


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------------------
def batches(env, kernel, nq, counts):
    c = tt.case(nb=max(counts), nq=nq, **tt.TINY_TABLES)
    longest = None
    for nb in sorted(counts, reverse=True):
        got = run(env, c, 'exp10' if nb == max(counts) else None, 'nbatch', kernels=(kernel,), nb=nb)[kernel]
        if longest is None:
            longest = run(env, c, None, 'nbatch', kernels=(kernel,), nb=nb)[kernel]
        else:
            assert same_bits(got, longest[:nb]), 'the first %d tables of a longer batch: other bits' % nb


@pytest.mark.parametrize('nq', sorted(tt.DIRECT_BATCHES))
def test_direct_batches(env, nq):
    """Around the 2048 workgroups from which a workgroup strides over tables: one tile per row, and three tiles (a grid of 2046)."""
    batches(env, 'direct', nq, tt.DIRECT_BATCHES[nq])


@pytest.mark.parametrize('nq', sorted(tt.ROWS_BATCHES))
def test_rows_batches(env, nq):
    """Around cp_tables_rows' cap of 512 workgroups: items of one tile and of two tiles per row."""
    batches(env, 'rows', nq, tt.ROWS_BATCHES[nq])


# ---- epilogues -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', tt.SCALES)
@pytest.mark.parametrize('post', [None, 'sqrt', 'exp10'])
def test_post_and_scale(env, post, scale):
    """The root of a negative element is NaN in that element only ('signed' tables: negative in the tail of every row)."""
    c = tt.case(scale=scale, kind='signed' if post == 'sqrt' else 'plain', nzq=64, nq=80, zq='inside')
    if post == 'sqrt':
        negative = c['truth'] < 0
        assert negative.any() and not negative.all()
    run(env, c, post, 'post')


@pytest.mark.parametrize('post', [None, 'sqrt', 'exp10'])
def test_nan_entry_stays_in_its_table(env, post):
    """A NaN in one entry of table 1: every other table keeps its bits.  Direct kernel (the NaN in y alone, M of the clean table): NaN in the columns of the
    two intervals at that knot, all redshifts; the other columns of those tiles of 16 within the allowance (with 10^x the wave leaves the table-driven
    form: the kernel's contract), every other tile the clean bits.  cp_tables_rows: NaN in whole columns, at least those, the rest within the allowance."""
    c = tt.case(nzq=64, nq=128, zq='inside')
    zi, j = 2, 13
    clean = run(env, c, post, 'nan')
    t = c['t'].copy()
    t[1, zi, j] = np.nan
    got = run(env, c, post, 'nan', t=t, judge=False)
    interval = np.clip(np.searchsorted(c['x'], c['xq'], side='right') - 1, 0, c['x'].size - 2)
    touched = (interval == j - 1) | (interval == j)
    assert touched.any() and not touched.all()
    for kernel in KERNELS:
        g = got[kernel]
        assert same_bits(np.delete(g, 1, axis=0), np.delete(clean[kernel], 1, axis=0)), '%s: the NaN reached another table' % kernel
        nan_columns = np.isnan(g[1]).any(axis=0)
        assert np.array_equal(np.isnan(g[1]), np.broadcast_to(nan_columns, g[1].shape)), '%s: NaN in parts of a column' % kernel
        if kernel == 'direct':
            assert np.array_equal(nan_columns, touched)
            tiles = np.repeat(touched.reshape(-1, 16).any(axis=1), 16)
            assert same_bits(g[1][:, ~tiles], clean[kernel][1][:, ~tiles]), 'a tile without the NaN: other bits'
        else:
            assert (nan_columns | ~touched).all()      # (the not-a-knot operator reaches every knot: the whole table may be NaN)
        expected = dict(c, truth=np.where(nan_columns[None, None, :] & (np.arange(3) == 1)[:, None, None], np.nan, c['truth']))
        assert note(kernel, 'nan', tt.fraction(g, expected, post, '%s, NaN entry, post %s' % (kernel, post))) <= 1.


@pytest.mark.parametrize('negative_scale', [False, True])
@pytest.mark.parametrize('nq', sorted(tt.BUMP_TILE))
@pytest.mark.parametrize('name', list(tt.EXPONENT_TARGETS))
def test_exponent_route(env, name, nq, negative_scale):
    """One tile of 16 wavenumbers x 64 redshifts with its largest |argument| at 299.9, 300 - 1 ulp, 300, 300.1, beyond 308.25 (Inf), in the subnormal range, below
    -324 (0); every other tile below 299.  The direct kernel switches a wave from the table-driven 10^x to the general one at 300: next to 300 either
    form is within the allowance; at 299.9 and 300.1 the route itself is held -- with 63 output redshifts no tile is ``full`` and every element takes the
    general form on the same arguments: at 300.1 the bump's tile has those bits, at 299.9 it has not (nor have the others)."""
    c = tt.exponent_case(name, nq, negative_scale)
    got = run(env, c, 'exp10', 'exponent')
    lo = 16 * c['tile']
    bump = got['direct'][:, :, lo:lo + 16]
    if name == 'inf':
        assert np.isinf(bump).any() and np.isfinite(np.delete(got['direct'], np.arange(lo, lo + 16), axis=2)).all()
    if name == 'zero':
        assert (bump == 0).any() and ((bump > 0) & (bump < 2.3e-308)).any()
    if name == 'subnormal':
        assert ((bump > 0) & (bump < 2.3e-308)).any() and (bump > 0).all()
    if name in ('299.9', '300.1'):
        P63 = plans(env, c, zq=c['zq'][:63])
        general = call(env, 'direct', P63, c['t'], 2, 'exp10', c['scale'], nzq=63)
        same = got['direct'][:, :63] == general
        rest = np.delete(same, np.arange(lo, lo + 16), axis=2)
        assert not rest.all(), 'no tile below 299 took the table-driven form'
        if name == '300.1':
            assert same[:, :, lo:lo + 16].all(), 'a tile that holds |argument| >= 300 did not take the general form'
        else:
            assert not same[:, :, lo:lo + 16].all(), 'a tile below 300 did not take the table-driven form'


@pytest.mark.parametrize('nq', tt.WIDE_NQ)
def test_a_million_wavenumbers(env, nq):
    """nq = 2^20 and 2^20 + 16, either side of the row length up to which a full tile takes the table-driven 10^x (its 32-bit store offsets): one table, 0.5 GB
    of output; sentinels, NaN and the bits of two calls and both layouts over the whole array, the truth on 5120 columns."""
    c = tt.wide_case(nq)
    got = run(env, c, 'exp10', 'wide', kernels=('direct',), judge=False)['direct']
    assert not np.isnan(got).any() and (got > 0).all()
    assert note('direct', 'wide', tt.fraction(got[:, :, c['cols']], c, 'exp10', 'direct, %d wavenumbers' % nq)) <= 1.


def test_worst_fractions():
    for key in sorted(WORST):
        print('MEASURED %-6s %-10s %.3f' % (key + (WORST[key],)))
