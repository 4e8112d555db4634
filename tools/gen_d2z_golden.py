"""Fixture of the batched DistanceToRedshift: tests/golden/distance_to_redshift_batch.npz, the outputs of the reference's own ``DistanceToRedshift``
for eight cosmologies (build machine only: the reference is imported as oracle/gen_golden.py imports it; no test imports this file).

    python tools/gen_d2z_golden.py

Per setting s = (zmax, nz, interp_order) of SETTINGS: ``rgrid_<zmax>_<nz>`` (B, nz), the reference's own table ``comoving_radial_distance(zgrid)``
(shared by settings that differ in the order only); ``d_<s>`` (B, NQ) distances per cosmology -- both end knots, a few interior knots, the rest uniform in the
table's range -- with ``z_<s>`` (B, NQ) the reference's redshifts there; ``ds_<s>`` (NQS,) distances inside every cosmology's table with ``zs_<s>`` (B, NQS).
The parameters of the cosmologies are stored under their names."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [(100., 512, 3), (10., 4096, 3), (100., 512, 1)]
NQ, NQS = 512, 256
# Omega_m, h, (w0, wa), Omega_k of both signs; one massive neutrino species of varying mass
PARAMS = dict(Omega_m=[0.31, 0.25, 0.40, 0.28, 0.35, 0.30, 0.27, 0.33], h=[0.68, 0.6, 0.8, 0.7, 0.72, 0.65, 0.75, 0.67],
              w0_fld=[-1., -1., -0.9, -1., -1.1, -1., -0.7, -0.8], wa_fld=[0., 0., 0.2, 0., -0.3, 0., -0.5, 0.1],
              Omega_k=[0., 0.05, -0.05, 0.1, -0.1, 0.01, -0.02, 0.], m_ncdm=[0.06, 0.06, 0.1, 0.2, 0.06, 0.3, 0.15, 0.08])
ENGINE = 'eisenstein_hu'


def tag(setting):
    return '%d_%d_%d' % setting


def main():
    from oracle._refimport import import_reference
    cp = import_reference()
    from cosmoprimo.utils import DistanceToRedshift
    warnings.simplefilter('ignore')
    nb = len(PARAMS['h'])
    out = {name: np.array(v, dtype='f8') for name, v in PARAMS.items()}
    rng = np.random.default_rng(42)
    cosmos = [cp.Cosmology(engine=ENGINE, **{name: ([float(v[i])] if name == 'm_ncdm' else float(v[i])) for name, v in PARAMS.items()}) for i in range(nb)]
    for setting in SETTINGS:
        zmax, nz, order = setting
        zgrid = 1. / np.geomspace(1. / (1. + zmax), 1., nz)[::-1] - 1.      # DistanceToRedshift's own grid
        objs, rgrid = [], []
        for cosmo in cosmos:
            ba = cosmo.get_background()
            objs.append(DistanceToRedshift(ba.comoving_radial_distance, zmax=zmax, nz=nz, interp_order=order))
            r = np.asarray(ba.comoving_radial_distance(zgrid), dtype='f8')
            assert np.isfinite(r).all() and (np.diff(r) > 0.).all(), 'table of a fixture cosmology not finite and ascending'
            assert np.array_equal(r, np.asarray(objs[-1]._interp._x)), 'the stored table is not the one the reference interpolates'
            rgrid.append(r)
        rgrid = np.array(rgrid)
        out['rgrid_%d_%d' % (zmax, nz)] = rgrid
        d = rgrid[:, :1] + rng.uniform(0., 1., (nb, NQ)) * (rgrid[:, -1:] - rgrid[:, :1])
        knots = [0, nz - 1, 1, nz - 2, nz // 2, nz // 3, 7]
        d[:, :len(knots)] = rgrid[:, knots]
        d = np.clip(d, rgrid[:, :1], rgrid[:, -1:])
        ds = np.sort(rng.uniform(rgrid[:, 0].max(), rgrid[:, -1].min(), NQS))
        ds[0], ds[-1] = rgrid[:, 0].max(), rgrid[:, -1].min()
        z = np.array([obj(d[i]) for i, obj in enumerate(objs)])
        zs = np.array([obj(ds) for obj in objs])
        assert np.isfinite(z).all() and np.isfinite(zs).all()
        out['d_' + tag(setting)], out['z_' + tag(setting)], out['ds_' + tag(setting)], out['zs_' + tag(setting)] = d, z, ds, zs
    path = os.path.join(ROOT, 'tests', 'golden', 'distance_to_redshift_batch.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
