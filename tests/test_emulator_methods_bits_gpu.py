"""GPU: the results of the derivative, objective, fit and sampling methods of ``Emulator``, bit for bit, against tests/golden/emulator_methods_bits.npz -- what
they gave before ``gauss_newton``, ``chi2_hessian``, ``least_squares`` and ``hmc`` were put behind one objective and ``jacobian`` / ``jvp`` / ``jvp2`` and
``vjp`` / ``vjp2`` behind one run loop each (recorded on an MI355X by tools/gen_emulator_methods_bits.py, every call run twice there and refused if its two
runs differed or held a value that is not finite).  That change touched no kernel and no launch argument, and the kernels use no atomics, so every output must be
EQUAL: a tolerance would not see two runs added in the other order, a precision permuted the other way or a mask applied once instead of twice.

The emulators, the batch and the three keys over the toy engines' 8 columns are those of tests/test_emulator_front_bits_gpu.py ``emulator_entries``: 'head.a'
(3,), 'head.b' (2, 2), 'tail' () and the fixed 'x', at B = 33 and at one point of scalar parameters, for every key (one run), the section 'head' (one run)
and 'head.a' with 'tail' (two runs); under a dense precision the keys are listed against the order of the columns, so that the permutation runs.  The inputs
come from seeded numpy (the data is the toy function itself at displaced points with 1 % of noise, never a prediction), so the file holds outputs only.  The
weight of the second entry of 'head.a' is exactly 0 -- the diagonal entry of the precision likewise -- and the datum under it NaN, in every call that takes
weights.  A value is stored once: what a method returns beside its result and must equal ``predict``'s, ``jvp``'s or ``gauss_newton``'s (the values, the first
derivatives of ``jvp2``, the Fisher matrix without data, the gradient and chi2 of ``chi2_hessian``, the default metric of ``hmc``) is compared with that here.
Integers are stored as float64 (exact), their type in the entry's name.  The file holds one flat float64 array per test and the names and shapes of its entries."""
import os

import numpy as np
import pytest

import mlp_reference as mr
from test_emulator_front_bits_gpu import _same, assert_equal_bits, flatten  # noqa: F401  (flatten: for tools/gen_emulator_methods_bits.py)
from test_emulator_jacobian_gpu import NAMES, XGRID, batch, emulators  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'emulator_methods_bits.npz')
B, AT = 33, 5
KEYS, SHAPES = ['head.a', 'head.b', 'tail'], [(3,), (2, 2), ()]
# (label, keys=, the varied keys that selects, the order a dense precision lists them in)
SELECTIONS = [('all', None, KEYS, ['tail', 'head.b', 'head.a']), ('section', 'head', ['head.a', 'head.b'], ['head.b', 'head.a']), ('two_runs', ['head.a', 'tail'], ['head.a', 'tail'], ['tail', 'head.a'])]


def split_emulator(emulator):
    """``emulator``'s engine under the three varied keys."""
    from cosmoprimo_amd.emulators import Emulator
    split = Emulator.__new__(Emulator)
    split.calculator, split.samples, split.params, split.fixed, split.engine = None, None, dict(emulator.params), {'x': XGRID}, emulator.engine
    split.varied_keys, split.varied_shapes = list(KEYS), list(SHAPES)
    return split


def inputs():
    """The operands of every call at B = 33, from seeded numpy: the start, tangents (one direction, and K = 2 twice), cotangents, weights, data and the (8,)
    inverse variances a dense precision is made of."""
    rng = np.random.default_rng(34)
    params = batch(B)
    truth = [params[name] + 0.03 * (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) * rng.uniform(-1., 1., B) for name in NAMES]
    Y = mr.toy(*truth)
    w = 1. / (1e-2 * np.abs(Y).mean(axis=0))**2
    Y = Y * (1. + 1e-2 * rng.standard_normal(Y.shape))
    data = {'head.a': Y[:, :3].copy(), 'head.b': Y[:, 3:7].reshape(B, 2, 2), 'tail': Y[:, 7].copy()}
    weights = {'head.a': w[:3] * rng.uniform(0.5, 2., (B, 3)), 'head.b': w[3:7].reshape(2, 2), 'tail': w[7]}      # per point, shared, a scalar
    weights['head.a'][:, 1], data['head.a'][:, 1] = 0., np.nan
    return {'params': params, 'data': data, 'weights': weights, 'w': w,
            'tangents': {'a': rng.normal(0., 1., B), 'b': 0.5, 'c': rng.normal(0., 1., B)},
            'tangentsK': {'a': rng.normal(0., 1., (B, 2)), 'b': rng.normal(0., 1., (1, 2)), 'c': rng.normal(0., 1., B)},
            'tangentsK2': {'a': rng.normal(0., 1., (1, 2)), 'c': rng.normal(0., 1., (B, 2))},      # no 'b': a zero component
            'cotangents': {key: rng.normal(0., 1., (B,) + shape) for key, shape in zip(KEYS, SHAPES)}}


def at_point(operands):
    """The operands of row AT alone, as a call with scalar parameters takes them: what varies with the point loses its leading axis (a (B, K) tangent keeps
    one, of length 1)."""
    def row(value, K=False):
        if np.shape(value)[:1] != (B,):      # shared by all points
            return value
        return value[AT:AT + 1] if K and np.ndim(value) == 2 else value[AT]
    out = {name: {key: row(value, K=name.startswith('tangentsK')) for key, value in operand.items()} for name, operand in operands.items() if name not in ('w', 'params')}
    out.update(w=operands['w'], params={name: float(operands['params'][name][AT]) for name in NAMES})
    return out


def dense_precision(w, listed):
    """P[c, d] = 0.6^|c - d| sqrt(w_c w_d) over the entries of the keys ``listed``, in that order; the diagonal entry of the second value of 'head.a' exactly 0."""
    columns = {'head.a': [0, 1, 2], 'head.b': [3, 4, 5, 6], 'tail': [7]}
    order = np.array([c for key in listed for c in columns[key]])
    c = np.arange(len(order))
    precision = 0.6**np.abs(c[:, None] - c[None, :]) * np.sqrt(w[order][:, None] * w[order][None, :])
    masked = int(np.flatnonzero(order == 1)[0])
    precision[masked, masked] = 0.
    return precision


def _store(out, name, value):
    if isinstance(value, dict):      # by parameter name: the last axis
        assert list(value) == NAMES, (name, list(value))
        value = np.stack([np.asarray(value[n]) for n in NAMES], axis=-1)
    value = np.asarray(value)
    if value.dtype != np.float64:
        name, value = '%s:%s' % (name, value.dtype), value.astype('f8')
    out[name] = value


def _same_values(values, want, keys):
    return [key for key in values if key != 'x'] == keys and all(_same(values[key], want[key]) for key in values)


def method_entries(emulator):
    """Every call the module's docstring names, on ``emulator``'s engine: ``{'<batch or point>.<selection>.<call>.<result>': array}``."""
    split = split_emulator(emulator)
    batched = inputs()
    out = {}
    for label, op in (('batch', batched), ('point', at_point(batched))):
        p = op['params']
        for what, keys, wanted, listed in SELECTIONS:
            got = {}
            predict = split.predict(p, keys=keys)
            # forward mode
            values, got['jvp'] = split.jvp(p, op['tangents'], keys=keys, return_value=True)
            assert list(values) == list(predict) and _same_values(values, predict, wanted)
            values, got['jvpK'] = split.jvp(p, op['tangentsK'], keys=keys, return_value=True)
            assert list(values) == list(predict) and _same_values(values, predict, wanted)
            values, first, got['jvp2'] = split.jvp2(p, op['tangents'], keys=keys, return_value=True, return_first=True)
            assert list(values) == list(predict) and _same_values(values, predict, wanted) and _same_values(first, got['jvp'], wanted)
            values, first, first2, got['jvp2K'] = split.jvp2(p, op['tangentsK'], op['tangentsK2'], keys=keys, return_value=True, return_first=True)
            assert list(values) == list(predict) and _same_values(values, predict, wanted) and _same_values(first, got['jvpK'], wanted)
            assert _same_values(first2, split.jvp(p, op['tangentsK2'], keys=keys), wanted)
            got['hessian'] = split.hessian(p, keys=keys)
            for name, result in got.items():
                assert list(result) == wanted, (label, what, name, list(result))
                for key in wanted:
                    _store(out, '%s.%s.%s.%s' % (label, what, name, key), result[key])
            # reverse mode and the objective: the keys of the operands select
            predict = split.predict(p, keys=wanted)
            weights, data = ({key: op[name][key] for key in wanted} for name in ('weights', 'data'))
            values, hess = split.vjp2(p, {key: op['cotangents'][key] for key in wanted}, return_value=True)
            assert _same_values(values, predict, wanted)
            _store(out, '%s.%s.vjp2' % (label, what), hess)
            for route, w, kwargs in (('diagonal', weights, {}), ('dense', listed, {'precision': dense_precision(op['w'], listed)})):
                prefix = '%s.%s.%s.' % (label, what, route)
                values, fisher, gradient, chi2 = split.gauss_newton(p, w, data=data, return_value=True, **kwargs)
                assert _same_values(values, predict, wanted)
                values, only = split.gauss_newton(p, w, return_value=True, **kwargs)
                assert _same_values(values, predict, wanted) and _same(only, fisher)
                for name, result in (('fisher', fisher), ('gradient', gradient), ('chi2', chi2)):
                    _store(out, prefix + 'gauss_newton.' + name, result)
                values, hess, g, c = split.chi2_hessian(p, w, data, return_value=True, **kwargs)
                assert _same_values(values, predict, wanted) and list(g) == NAMES and all(_same(g[name], gradient[name]) for name in NAMES) and _same(c, chi2)
                _store(out, prefix + 'chi2_hessian', hess)
                for name, options in (('least_squares', {}), ('least_squares_geodesic', {'geodesic': True})):
                    if route == 'dense' and not options:      # three fits: plain, geodesic, geodesic under the precision
                        continue
                    best, c, info = split.least_squares(p, w, data, niterations=4, **options, **kwargs)
                    for result, value in [('best', best), ('chi2', c)] + [('info.' + key, value) for key, value in info.items()]:
                        _store(out, prefix + name + '.' + result, value)
                samples, c, info = split.hmc(p, w, data, nsamples=3, nwarmup=1, thin=2, nleapfrog=3, **kwargs)
                assert _same(info.pop('metric'), fisher)      # the start is inside the box: the default metric is gauss_newton's there
                for result, value in [('samples', samples), ('chi2', c)] + [('info.' + key, value) for key, value in info.items()]:
                    _store(out, prefix + 'hmc.' + result, value)
    return out


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_methods(recorded, emulators, which):  # noqa: F811
    assert_equal_bits(method_entries(emulators[which]), recorded, 'methods_%s' % which)
