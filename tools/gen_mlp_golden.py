"""Fixture of the MLP emulator: tests/golden/mlp.npz, the reference's own predictions for networks with seeded weights and its quasi-random points
(build machine only: the reference is imported as oracle/gen_golden.py imports it; no test imports this file).

    python tools/gen_mlp_golden.py

The file holds numbers and the names of activations and operations only.  The reference keeps a network as a list of steps, each an expression it
evaluates; the generator takes those expressions from the reference's own source at run time (the arguments of the ``Operation(...)`` calls in
``ExplicitMLP.operations``, found with :mod:`ast`), binds the weights to them as ``mlp.py:192-216`` does and calls the reference's ``predict``, which
runs under numpy.  Nothing of them is written to the fixture or kept here.

Per configuration i of CONFIGS (keys ``c<i>_<name>``): ``nhidden``, ``activation`` (names, one per hidden layer), ``yfunction`` ('' / 'log10'), ``xkind`` /
``ykind`` ('scale' / 'norm'), ``parameters`` (the packed buffer: per layer kernel, bias and, for a hidden layer, alpha, beta), ``xoffset`` / ``xscale``
(3,), ``yoffset`` / ``yscale`` (M,) with ``(v - offset) / scale`` the forward operation, ``Xq`` (33, 3) raw query points and ``Yq`` (33, M) the reference's
``engine.predict`` at each.  ``qmc_<engine>`` (64, 3): the reference's ``QMCSampler`` points for 'rqrs', 'halton', 'sobol' (``QMC_SEED``) over ``limits``."""
import ast
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ('a', 'b', 'c')
LIMITS = {'a': (0.8, 1.2), 'b': (1.8, 2.2), 'c': (0.4, 0.6)}
# nhidden, activation, M, first y operation, kind of the last x / y operation
CONFIGS = [((32, 32, 32), 'silu', 8, None, 'scale'), ((64,), 'relu', 300, None, 'scale'), ((5, 17), 'tanh', 8, None, 'norm'),
           ((32, 32, 32), 'identity-silu', 300, 'log10', 'scale'), ((5, 17), ('identity-silu', 'silu'), 8, 'log10', 'norm'),
           ((32, 32, 32), ('tanh', 'relu', 'silu'), 300, None, 'scale')]
NQUERIES, NSAMPLES, QMC_SEED = 33, 50, 7


def reference_expressions(path):
    """{'dense' | activation name: expression} from the reference's ``operations`` method."""
    tree = ast.parse(open(path).read())
    func = [node for node in ast.walk(tree) if isinstance(node, ast.FunctionDef) and node.name == 'operations'][0]
    found = {}

    def first_string(call):
        return call.args[0].value

    for node in ast.walk(func):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and isinstance(node.test.left, ast.Name) and node.test.left.id == 'activation':
            calls = [c for c in ast.walk(ast.Module(body=node.body, type_ignores=[])) if isinstance(c, ast.Call) and getattr(c.func, 'id', '') == 'Operation']
            found[node.test.comparators[0].value] = first_string(calls[0])
        if isinstance(node, ast.Call) and getattr(node.func, 'id', '') == 'Operation' and any(isinstance(kw.value, ast.DictComp) for kw in node.keywords):
            found['dense'] = first_string(node)
    assert set(found) == {'dense', 'silu', 'relu', 'tanh', 'identity-silu'}, sorted(found)
    return found


def main():
    from oracle._refimport import import_reference, REFERENCE_ROOT
    import_reference()
    from cosmoprimo.emulators.tools import mpi
    from cosmoprimo.emulators.tools.base import Operation
    from cosmoprimo.emulators.tools.mlp import MLPEmulatorEngine
    from cosmoprimo.emulators.tools.samples import QMCSampler
    from cosmoprimo_amd.emulators.tools.mlp import pack_parameters
    warnings.simplefilter('ignore')
    expressions = reference_expressions(os.path.join(REFERENCE_ROOT, 'cosmoprimo', 'emulators', 'tools', 'mlp.py'))
    rng = np.random.default_rng(42)
    limits = np.array([LIMITS[name] for name in NAMES])
    out = {'names': np.array(NAMES), 'limits': limits}
    for i, (nhidden, activation, M, yfunction, kind) in enumerate(CONFIGS):
        engine = MLPEmulatorEngine(nhidden=nhidden, activation=activation, xoperation=kind, yoperation=[op for op in (yfunction, kind) if op])
        engine.initialize(list(NAMES), mpicomm=mpi.COMM_WORLD)
        # samples to initialise the operations on: the x limits come out as the box, one y column has zero spread
        X = rng.uniform(limits[:, 0], limits[:, 1], (NSAMPLES, 3))
        X[0], X[1] = limits[:, 0], limits[:, 1]
        Y = rng.uniform(0.5, 3., (NSAMPLES, M)) * np.geomspace(1e-2, 1e3, M)
        Y[:, 2] = 1.      # (a value whose mean, and the mean of whose log10, are exact: the standard deviation is exactly 0)
        values = Y
        for operation in engine.yoperations:
            operation.initialize(values)
            values = np.array([operation(v) for v in values])
        values = X
        for operation in engine.xoperations:
            operation.initialize(values)
            values = np.array([operation(v) for v in values])
        engine.xshape, engine.yshape = (3,), (M,)
        dims = (3,) + tuple(nhidden) + (M,)
        layers, operations = [], []
        for l in range(len(dims) - 1):
            layer = {'kernel': rng.normal(0., 1., (dims[l], dims[l + 1])) / np.sqrt(dims[l]), 'bias': rng.normal(0., 0.3, dims[l + 1])}
            operations.append(Operation(expressions['dense'], locals={name: layer[name] for name in ['kernel', 'bias']}))
            if l < len(nhidden):
                name = engine.activation[l]
                layer['alpha'], layer['beta'] = (rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.8)) if name == 'identity-silu' else (0., 0.)
                operations.append(Operation(expressions[name], locals={'beta': np.asarray(layer['beta']), 'alpha': np.asarray(layer['alpha'])} if name == 'identity-silu' else {}))
            layers.append(layer)
        engine.model_operations = operations
        Xq = rng.uniform(limits[:, 0], limits[:, 1], (NQUERIES, 3))
        Xq[0], Xq[1] = limits.mean(axis=1), limits[:, 1]
        Yq = np.array([np.asarray(engine.predict(dict(zip(NAMES, xq))), dtype='f8') for xq in Xq])
        assert Yq.shape == (NQUERIES, M) and np.isfinite(Yq).all()

        def affine(operation):
            loc = operation.locals
            return (loc['limits'][0], loc['limits'][1] - loc['limits'][0]) if operation.name == 'scale' else (loc['mean'], loc['sigma'])

        (xoffset, xscale), (yoffset, yscale) = affine(engine.xoperations[-1]), affine(engine.yoperations[-1])
        assert [op.name for op in engine.xoperations] == [kind] and [op.name for op in engine.yoperations] == [op for op in (yfunction, kind) if op]
        assert yoffset[2] == (0. if kind == 'scale' or yfunction else 1.) and yscale[2] == 1.      # the column with zero spread
        state = dict(nhidden=np.array(nhidden, dtype='i8'), activation=np.array(engine.activation), yfunction=np.array(yfunction or ''), xkind=np.array(kind),
                     ykind=np.array(kind), parameters=pack_parameters(layers), xoffset=np.asarray(xoffset, dtype='f8'), xscale=np.asarray(xscale, dtype='f8'),
                     yoffset=np.asarray(yoffset, dtype='f8'), yscale=np.asarray(yscale, dtype='f8'), Xq=Xq, Yq=Yq)
        for name, value in state.items():
            out['c%d_%s' % (i, name)] = value
    for name in ('rqrs', 'halton', 'sobol'):
        sampler = QMCSampler(None, params=dict(LIMITS), engine=name, mpicomm=mpi.COMM_WORLD, seed=0.5 if name == 'rqrs' else QMC_SEED)
        if name == 'sobol':      # the reference's ``_points`` calls ``fast_forward(0)``, which this scipy's Sobol refuses (it converts -1 to unsigned); skipping 0 points
            from scipy.stats import qmc      # is no operation, so its remaining steps are taken here: reset, ``random``, ``qmc.scale``
            sampler.engine.reset()
            out['qmc_' + name] = qmc.scale(sampler.engine.random(n=64), limits[:, 0], limits[:, 1])
        else:
            points = sampler.points(niterations=64)
            out['qmc_' + name] = np.column_stack([np.asarray(points[n], dtype='f8') for n in NAMES])
        assert out['qmc_' + name].shape == (64, 3)
    out['qmc_seed'] = np.array(QMC_SEED)
    path = os.path.join(ROOT, 'tests', 'golden', 'mlp.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
