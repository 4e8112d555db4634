"""Fixture of the Taylor emulator: tests/golden/taylor.npz, the reference's own finite-difference grids, Taylor coefficients and predictions for a toy
function (build machine only: the reference is imported as oracle/gen_golden.py imports it; no test imports this file).

    python tools/gen_taylor_golden.py

The toy is f(a, b, c) = concat(exp(a x) sin(b x) + c^3 x, [a b c]) on x = linspace(0.1, 1, 7): M = 8 outputs, none of them a polynomial the
expansion would reproduce exactly except the last.  The reference's ``DiffSampler.run()`` and ``mpi.bcast`` need mpi4py, which this machine does not
have: the generator takes ``DiffSampler(...).points()``, evaluates the toy itself, makes ``mpi.bcast`` the identity for the run and calls
``TaylorEmulatorEngine._fit_no_operation`` / ``_predict_no_operation`` directly.

Per configuration i of CONFIGS (keys ``c<i>_<name>``): ``X`` (npoints, 3) the sample matrix in the reference's order, ``Y`` (npoints, 8), ``cidx``,
``order`` and ``accuracy`` (3,) per parameter, ``center`` (3,), ``powers`` (T, 3), ``derivatives`` (T, 8), ``Xq`` (33, 3) query points (uniform in the
limits, the centre first and one corner second) and ``Yq`` (33, 8) the reference's prediction at each.  ``limits`` (3, 2) and ``names`` are shared."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ('a', 'b', 'c')
LIMITS = {'a': (0.8, 1.2), 'b': (1.8, 2.2), 'c': (0.4, 0.6)}
# (order, accuracy) -> the points and terms the reference gives
CONFIGS = [(3, 2, 33, 20), (4, 2, 57, 35), (2, 4, 61, 10), ({'a': 3, 'b': 1, 'c': 2}, 2, 17, 8), ({'a': 2, 'b': 0, 'c': 1}, 2, 9, 4)]
NQUERIES = 33


def toy(a, b, c):
    x = np.linspace(0.1, 1., 7)
    a, b, c = (np.asarray(v, dtype='f8')[..., None] for v in (a, b, c))
    return np.concatenate([np.exp(a * x) * np.sin(b * x) + c**3 * x, a * b * c], axis=-1)


def main():
    from oracle._refimport import import_reference
    import_reference()
    from cosmoprimo.emulators.tools import mpi
    from cosmoprimo.emulators.tools.samples import DiffSampler
    from cosmoprimo.emulators.tools.taylor import TaylorEmulatorEngine
    warnings.simplefilter('ignore')
    mpi.bcast = lambda value, *args, **kwargs: value
    rng = np.random.default_rng(42)
    out = {'names': np.array(NAMES), 'limits': np.array([LIMITS[name] for name in NAMES])}
    for i, (order, accuracy, npoints, nterms) in enumerate(CONFIGS):
        sampler = DiffSampler(None, params=dict(LIMITS), order=order, accuracy=accuracy)
        samples = sampler.points()
        X = np.column_stack([np.asarray(samples[name], dtype='f8') for name in NAMES])
        Y = toy(*X.T)
        engine = TaylorEmulatorEngine(order=order, accuracy=accuracy)
        engine.params, engine.mpicomm = list(NAMES), mpi.COMM_WORLD
        engine._fit_no_operation(X, Y, samples.attrs)
        center, powers, derivatives = (np.asarray(v) for v in (engine.center, engine.powers, engine.derivatives))
        assert X.shape == (npoints, 3) and powers.shape == (nterms, 3) and derivatives.shape == (nterms, 8), (X.shape, powers.shape)
        Xq = rng.uniform(out['limits'][:, 0], out['limits'][:, 1], (NQUERIES, 3))
        Xq[0], Xq[1] = center, out['limits'][:, 1]
        Yq = np.array([np.asarray(engine._predict_no_operation(xq), dtype='f8') for xq in Xq])
        assert np.isfinite(Yq).all() and np.array_equal(Yq[0], Y[samples.attrs['cidx'][0]])
        state = dict(X=X, Y=Y, cidx=np.array(samples.attrs['cidx'], dtype='i8'), order=np.array([samples.attrs['order'][name] for name in NAMES], dtype='i8'),
                     accuracy=np.array([samples.attrs['accuracy'][name] for name in NAMES], dtype='i8'), center=center.astype('f8'), powers=powers.astype('i8'),
                     derivatives=derivatives.astype('f8'), Xq=Xq, Yq=Yq)
        for name, value in state.items():
            out['c%d_%s' % (i, name)] = value
    path = os.path.join(ROOT, 'tests', 'golden', 'taylor.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
