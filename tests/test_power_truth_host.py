"""CPU: tests/power_truth.py, the restatement that tests/test_power_truth_gpu.py holds the analytic power-spectrum kernels to.

1. Its float64 form equals ``oracle.power``, which cites the reference line by line.  Bit for bit (the same expressions on arrays of the same shapes):
   ``eh_scalars`` with ``alpha_gamma``, ``bbks_gamma``, ``transfer_eh``, ``transfer_nowiggle``, ``transfer_bbks``, ``primordial_pk``, ``pk_callable``.
   To 2 ulp, the bound met (``variants_scalars``, whose oracle works on the scalars of one cosmology: numpy's scalar pow and its array pow differ in the last bit) and
   to rtol = 2e-15 (``variants_transfer_kz``, which takes those scalars through six more powers).
2. Every block of every device case lies below its cap (32 floors; 64 for ``matter`` and ``log_k_matter``); the cases are built by the functions of
   tests/power_truth.py that the device tests call.
3. The BBKS weight is justified by measurement: without it the decades below k = 1e-4 h/Mpc are over the cap (7e6 floors for the transfer function, 1.5e7
   for the spectrum, growing as 1 / k), with it they are under (at the floor).
4. The rule rejects the neighbours: the float64 restatement with one mutation stands in for the device and fails ``assert_pointwise``.
5. ``split_wavenumbers`` and the block size restated: the documented examples, and every case reaches the edge of the launch it is named for."""
import numpy as np
import pytest

import background_truth as bt
import power_truth as pt
from oracle import power as opw

F8 = np.float64
EH, NW, BBKS = pt.ENGINES


def same(a, b):
    a, b = np.asarray(a, dtype='f8'), np.asarray(b, dtype='f8')
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def parameters(n=40, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.6, 0.8, n), rng.uniform(0.15, 0.35, n), rng.uniform(0.03, 0.06, n), rng.uniform(2.6, 2.8, n)


K = np.concatenate([np.geomspace(1e-8, 1e5, 300), np.linspace(7e-5, 7., 100)])


def test_float64_restatement_equals_oracle():
    h, Omega_cdm, Omega_b, T_cmb = parameters()
    mine, theirs = pt.eh_scalars(h, Omega_cdm, Omega_b, T_cmb, F8), opw.eh_scalars(h, Omega_cdm, Omega_b, T_cmb)
    assert set(mine) == set(theirs)
    for name in theirs:
        assert same(mine[name], theirs[name]), name
    nu = np.random.default_rng(6).uniform(0., 0.01, h.size)
    gamma = pt.bbks_gamma(h, Omega_cdm, Omega_b, nu, F8)
    assert same(gamma, opw.bbks_gamma(h, Omega_cdm, Omega_b, nu))
    assert same(pt.transfer_eh(K, h, mine, F8), opw.transfer_eh(K, h, theirs))
    assert same(pt.transfer_nowiggle(K, h, mine, F8), opw.transfer_nowiggle(K, h, theirs))
    assert same(pt.transfer_bbks(K, h, gamma, F8), opw.transfer_bbks(K, h, gamma))
    pk = pt.primordial_parameters(h.size, 7)
    prim = pt.primordial_pk(K, h, *pk.T, dtype=F8)
    assert same(prim, opw.primordial_pk(K, h, *pk.T))
    T = pt.transfer_eh(K, h, mine, F8)
    assert same(pt.pk_callable(K, T, Omega_b + Omega_cdm + nu, h, prim, F8), opw.pk_callable(K, T, Omega_b + Omega_cdm + nu, h, prim))
    x = np.linspace(-3., 3., 61)
    assert same(pt.sinc(x), np.sinc(x)) and pt.sinc(np.zeros(1, dtype=bt.LD))[0] == 1


@pytest.mark.parametrize('nsp', [0, 1, 3])
def test_float64_variants_equal_oracle(nsp):
    h, Omega_cdm, Omega_b, T_cmb = parameters(6, 8 + nsp)
    rng = np.random.default_rng(9)
    Opn, Oppn = rng.uniform(1e-3, 4e-3, (6, nsp)), rng.uniform(1e-6, 1e-5, (6, nsp))
    mine = pt.variants_scalars(h, Omega_cdm, Omega_b, T_cmb, Opn, Oppn, F8)
    z, k = np.array([0., 0.5, 3.]), np.geomspace(1e-4, 30., 50)
    gk0 = rng.uniform(500., 3000., (6, 3))
    worst = 0.
    for i in range(6):
        p = dict(h=h[i], Omega_cdm=Omega_cdm[i], Omega_b=Omega_b[i], T_cmb=T_cmb[i])
        if nsp:
            p.update(Omega_ncdm=Opn[i], Omega_pncdm=Oppn[i], m_ncdm=[0.1] * nsp)
        theirs = opw.variants_scalars(p)
        assert set(theirs) == set(mine)
        for name, v in theirs.items():
            if name == 'N_ncdm':
                assert v == mine[name] == nsp
                continue
            ulp = np.spacing(max(abs(v), abs(pt.ABSOLUTE_SCALARS.get(name, 0.))))
            worst = max(worst, abs(mine[name][i] - v) / ulp)
        for of in ('delta_m', 'delta_cb'):
            got = pt.variants_transfer_kz(k, h[i:i + 1], {n: (v if n == 'N_ncdm' else np.array([theirs[n]])) for n, v in mine.items()}, gk0[i:i + 1], of, F8)[0]
            np.testing.assert_allclose(got, opw.variants_transfer_kz(k, z, p, theirs, gk0[i], of=of).T, rtol=2e-15, atol=0)
    print('variants_scalars: at most %.3g ulp from the oracle' % worst)
    assert worst <= 2.


# ---- the caps -------------------------------------------------------------------------------------------------------------------------------------------

def both(fn, *args, **kwargs):
    return fn(*args, dtype=bt.LD, **kwargs), fn(*args, dtype=F8, **kwargs)


@pytest.mark.parametrize('index', range(len(pt.analytic_cases())))
def test_cap_analytic(index):
    case = pt.analytic_cases()[index]
    for engine in case['engines']:
        x = pt.case_x(case) if engine == BBKS else None
        for what in case['whats']:
            level = pt.level_floors(engine, what, case['k'], *both(pt.case_truth, case, engine, what), x=x)
            print('%s, %s %s: level at most %.3g FLOOR' % (case['name'], engine, what, level))
            assert level < pt.cap_of(what), (case['name'], engine, what)


@pytest.mark.parametrize('nsp', [0, 1, 3])
def test_cap_variants(nsp):
    for case in pt.variants_cases(nsp):
        for what in case['whats']:
            for of in ('delta_m', 'delta_cb'):
                level = pt.level_floors('variants', what, case['k'], *both(pt.variants_truth, case, what, of))
                print('%s, %s %s: level at most %.3g FLOOR' % (case['name'], what, of, level))
                assert level < pt.cap_of(what), (case['name'], what, of)


def scalar_levels(case):
    weights = pt.scalars_truth(case, 'eh', parts=True)
    out = {}
    for which, names in (('eh', pt.EH_SCALARS), ('variants', pt.VARIANTS_SCALARS)):
        ld, f8 = both(pt.scalars_truth, case, which)
        for name in names:
            _, t, f = pt.prepared_scalars([name], ld, ld, f8, weights)
            out[(which, name)] = float(bt.pointwise_level(t, f).max() / bt.FLOOR)
    return out


def test_cap_scalars():
    for n in pt.SCALAR_COUNTS:
        for nsp in (0, 3):
            levels = scalar_levels(pt.scalars_case(n, nsp))
            print('%d cosmologies, %d species: level at most %.3g FLOOR (%s)' % (n, nsp, max(levels.values()), max(levels, key=levels.get)[1]))
            assert max(levels.values()) < pt.CAP


def test_the_scales_of_the_scalars_are_needed():
    """alpha_b held against itself is over the cap (the sum inside alpha_b_G cancels to between 1 / 140 and 1 / 850 of its terms over these
    cosmologies); so are p_cb and frac_ncdm."""
    case = pt.scalars_case(257, 3)
    cl, c8 = pt.case_cosmo(case), pt.case_cosmo(case, F8)
    sl, s8 = pt.scalars_of(cl, parts=True), pt.scalars_of(c8)
    print('alpha_b: weights from %.3g to %.3g' % (sl['alpha_b_weight'].min(), sl['alpha_b_weight'].max()))
    assert 100. < sl['alpha_b_weight'].min() and sl['alpha_b_weight'].max() < 1000.
    assert bt.below_cap(sl['alpha_b'][:, None], s8['alpha_b'][:, None]) > pt.CAP
    vl, v8 = pt.variants_scalars(*pt.variants_inputs(cl)), pt.variants_scalars(*pt.variants_inputs(c8), dtype=F8)
    for name in ('p_cb', 'frac_ncdm'):
        assert bt.below_cap(vl[name][:, None], v8[name][:, None]) > pt.CAP, name


def test_the_bbks_weight_is_needed_and_enough():
    case = [c for c in pt.analytic_cases() if c['name'] == 'geomspace(1e-8, 1e2)'][0]
    k = case['k']
    low = k < 1e-4
    x = pt.case_x(case)
    for what in ('transfer', 'matter', 'log_k_matter'):
        ld, f8 = both(pt.case_truth, case, BBKS, what)
        unweighted = pt.level_floors(BBKS, what, k[low], ld[:, low], f8[:, low], weighted=False)
        weighted = pt.level_floors(BBKS, what, k[low], ld[:, low], f8[:, low], x=x[:, low])
        print('bbks %s below k = 1e-4: %.3g FLOOR unweighted, %.3g weighted' % (what, unweighted, weighted))
        assert unweighted > 100. * pt.cap_of(what) and weighted < pt.cap_of(what)
        # decade by decade the unweighted level grows as 1 / k
        per_decade = [pt.level_floors(BBKS, what, k[sel], ld[:, sel], f8[:, sel], weighted=False) for sel in ((k >= 10.**d) & (k < 10.**(d + 1)) for d in (-8, -6))]
        assert per_decade[0] > 10. * per_decade[1]


# ---- the neighbours -------------------------------------------------------------------------------------------------------------------------------------

def named(name):
    return [c for c in pt.analytic_cases() if c['name'] == name][0]


def rejected(engine, what, case, dev, truth, f64, why, x=None):
    pt.assert_quantity(engine, what, case['k'], f64, truth, f64, x, name=case['name'] + ', the restatement itself')
    with pytest.raises(AssertionError, match='of its allowance'):
        pt.assert_quantity(engine, what, case['k'], dev, truth, f64, x, name=case['name'] + ', ' + why)


@pytest.mark.parametrize('mutation', ['q108', 'no_beta_c', 'weight_swapped', 'sinc_without_pi'])
def test_the_rule_rejects_the_neighbours_of_eh98(mutation):
    case = named('3 cosmologies x 257 wavenumbers')
    for what in ('transfer', 'matter', 'log_k_matter'):
        ld, f8 = both(pt.case_truth, case, EH, what)
        rejected(EH, what, case, pt.case_truth(case, EH, what, F8, mutation=mutation), ld, f8, mutation)


def test_the_rule_rejects_the_neighbours_of_the_spectrum():
    case = named('3 cosmologies x 257 wavenumbers')
    for engine in pt.ENGINES:      # alpha_s / 2 -> alpha_s
        for what in ('primordial', 'matter', 'log_k_matter'):
            ld, f8 = both(pt.case_truth, case, engine, what)
            rejected(engine, what, case, pt.case_truth(case, engine, what, F8, mutation='alpha_s_whole'), ld, f8, 'alpha_s whole', x=pt.case_x(case))
    for engine in (EH, BBKS):      # Omega0_m without the massive species
        case = named('3 species, parameter 1 Omega_cdm, %s' % engine)
        ld, f8 = both(pt.case_truth, case, engine, 'matter')
        rejected(engine, 'matter', case, pt.case_truth(case, engine, 'matter', F8, mutation='no_nu_m'), ld, f8, 'Omega0_m without Omega_nu_m', x=pt.case_x(case))
    case = named('1 species, parameter 1 Omega_m, bbks')      # ... and the BBKS shape parameter
    ld, f8 = both(pt.case_truth, case, BBKS, 'transfer')
    rejected(BBKS, 'transfer', case, pt.case_truth(case, BBKS, 'transfer', F8, mutation='no_nu_m'), ld, f8, 'gamma without Omega_nu_m', x=pt.case_x(case))
    for name in ('3 cosmologies x 70 wavenumbers x 257 redshifts', '3072 cosmologies x 65 wavenumbers x 65 redshifts'):
        case = named(name)      # the growth factor of the neighbouring redshift: everywhere, and in the second block of redshifts alone
        block = pt.launch_shape(case['ncosmo'], case['nk'], case['nz'])['block']
        for engine in pt.ENGINES:
            ld, f8 = both(pt.case_truth, case, engine, 'matter')
            x = pt.case_x(case)
            rejected(engine, 'matter', case, np.roll(f8, 1, axis=1), ld, f8, 'the neighbouring redshift', x=x)
            dev = f8.copy()
            dev[:, block:] = f8[:, block - 1:-1]
            rejected(engine, 'matter', case, dev, ld, f8, 'the neighbouring redshift in the second block', x=x)
    case = named('3072 cosmologies x 341 wavenumbers')
    last = case['nk'] % 64
    assert last == 21
    shifted = dict(case, k=np.concatenate([case['k'][:-last], case['k'][-last + 1:], case['k'][-1:]]))
    for engine in pt.ENGINES:
        x = pt.case_x(case)
        for what in pt.WHATS:
            ld, f8 = both(pt.case_truth, case, engine, what)
            rejected(engine, what, case, np.roll(f8, 1, axis=0), ld, f8, 'the neighbouring cosmology', x=x)      # rows are sorted: a roll is the neighbour in the sample
            rejected(engine, what, case, pt.case_truth(shifted, engine, what, F8), ld, f8, 'k[i + 1] in the last %d entries' % last, x=x)


def test_the_rule_rejects_the_neighbours_of_the_variants():
    case = pt.variants_cases(3)[1]
    for what in ('transfer', 'matter'):
        ld, f8 = both(pt.variants_truth, case, what, 'delta_m')
        for why, dev in (('of swapped', pt.variants_truth(case, what, 'delta_cb', F8)), ('yfs left out', pt.variants_truth(case, what, 'delta_m', F8, mutation='no_yfs')),
                         ('the neighbouring redshift', np.roll(f8, 1, axis=1)), ('the neighbouring cosmology', np.roll(f8, 1, axis=0))):
            rejected('variants', what, case, dev, ld, f8, why)


def test_the_rule_rejects_the_neighbours_of_the_scalars():
    case = pt.scalars_case(257, 3)
    cl, c8 = pt.case_cosmo(case), pt.case_cosmo(case, F8)
    sl, s8 = pt.scalars_of(cl, parts=True), pt.scalars_of(c8)
    for name in pt.EH_SCALARS:      # every scalar one part in 1e13 off: 40 times the largest allowance (16 x 32 floors is 5.6e-14)
        dev = dict(s8, **{name: s8[name] * (1. + 1e-13 * (sl['alpha_b_weight'].astype(F8) if name == 'alpha_b' else 1.))})
        bt.assert_pointwise(*pt.prepared_scalars([name], s8, sl, s8, sl), name)
        with pytest.raises(AssertionError, match='of its allowance'):
            bt.assert_pointwise(*pt.prepared_scalars([name], dev, sl, s8, sl), name)
    no_nu = dict(s8, gamma=pt.bbks_gamma(c8['h'], c8['Omega_cdm'], c8['Omega_b'], 0., F8))
    with pytest.raises(AssertionError, match='of its allowance'):
        bt.assert_pointwise(*pt.prepared_scalars(['gamma'], no_nu, sl, s8, sl), 'gamma without Omega_nu_m')
    vl, v8 = pt.variants_scalars(*pt.variants_inputs(cl)), pt.variants_scalars(*pt.variants_inputs(c8), dtype=F8)
    Opn, Oppn = pt.omega_nu_m(c8)
    wrong = pt.variants_scalars(c8['h'], c8['Omega_cdm'], c8['Omega_b'], c8['T_cmb'], Opn, 0. * Oppn, F8)      # omega_m without the pressure term
    for name in ('omega_m', 'frac_ncdm', 'p_cb', 'gamma_ncdm', 'rs_drag'):
        bt.assert_pointwise(*pt.prepared_scalars([name], v8, vl, v8, sl), name)
        with pytest.raises(AssertionError, match='of its allowance'):
            bt.assert_pointwise(*pt.prepared_scalars([name], wrong, vl, v8, sl), name)


# ---- the launch shapes ----------------------------------------------------------------------------------------------------------------------------------

def test_launch_shapes():
    a = pt.launch_shape(1024, 1100)
    assert (a['block'], a['kspan'], a['kchunks']) == (256, 768, 2) and a['edges']['partial_pass'] and a['edges']['partial_chunk']
    b = pt.launch_shape(3072, 341)
    assert (b['block'], b['kspan'], b['kchunks']) == (64, 384, 1)
    assert pt.launch_shape(3071, 341)['block'] == 256 and pt.launch_shape(3072, 341, variants=True)['block'] == 256
    assert pt.split_wavenumbers(10000, 1024, 64) == (1024, 1, 16)      # a batch that fills the chip: all of a cosmology's wavenumbers


def test_every_case_reaches_its_edge():
    reached = set()
    for case in pt.analytic_cases():
        edges = pt.launch_shape(case['ncosmo'], case['nk'], case['nz'])['edges']
        assert all(edges[e] for e in case['edges']), (case['name'], edges)
        reached |= set(case['edges'])
        assert case['rows'][0] == 0 and case['rows'][-1] == case['ncosmo'] - 1 and (np.diff(case['rows']) > 0).all()
        if case['ncosmo'] >= 3071:
            assert len(case['rows']) == 32 and set((0, 1, 63, 64)) <= set(case['rows'].tolist())
        if case['kscale'] is not None:
            assert case['kscale'].min() >= 0.9 and case['kscale'].max() <= 1.1
            reached.add('kscale, one wave' if edges['one_wave'] else 'kscale, 256 threads')
        if case['z'] is not None:
            assert case['z'].min() == (0. if case['nz'] > 1 else 10.) and case['z'].max() == 10. and (case['nz'] < 3 or (np.diff(case['z']) > 0).any() and (np.diff(case['z']) < 0).any())
            if edges['z_blocks']:      # both launch shapes take a second block of redshifts
                reached.add('z_blocks, one wave' if edges['one_wave'] else 'z_blocks, 256 threads')
    assert reached == {'kiter', 'partial_pass', 'partial_chunk', 'z_blocks', 'one_wave', 'kscale, one wave', 'kscale, 256 threads', 'z_blocks, one wave',
                       'z_blocks, 256 threads'}
    kiter = named('kiter > 1: 1024 cosmologies x 1100 wavenumbers')
    assert len(kiter['rows']) == 24
    for nsp in (0, 1, 3):
        reached = set()
        for case in pt.variants_cases(nsp):
            edges = pt.launch_shape(case['ncosmo'], case['nk'], case['nz'], variants=True)['edges']
            assert all(edges[e] for e in case['edges']) and not edges['one_wave'], (case['name'], edges)
            reached |= set(case['edges'])
        assert reached == ({'z_blocks'} if nsp == 1 else {'z_blocks', 'kiter', 'partial_pass', 'partial_chunk'})
