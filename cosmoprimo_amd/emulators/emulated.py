"""
Emulated cosmological calculation under the reference's names (cosmoprimo/emulators/emulated.py): an engine whose sections are filled from a fitted
:class:`Emulator`, so that code written against :class:`Cosmology` runs on an emulator:

.. code-block:: python

    emulator.save(fn)
    cosmo = DESI(engine=EmulatedEngine.read(fn))                                             # one cosmology
    cosmo = Cosmology(engine=EmulatedEngine.read(fn), Omega_m=np.linspace(0.28, 0.34, 10000))  # a batch
    cosmo.get_background().comoving_radial_distance(z)                                       # (10000, nz)

A section is predicted when it is first asked for, and alone: ``Emulator.predict(params, keys=<section>, device=True)`` runs the engine on the columns of
that section (``cp_taylor_predict_columns`` / ``cp_mlp_predict_columns``), a (B, ncols) tensor that stays on the device -- the background of 10^4
cosmologies is 256 columns per table, not the 4 10^4 of every output.

Not built: the ``Harmonic`` section, emulators with ``z`` as a parameter (the reference's ``requires`` branch), emulator-level
``xoperations`` / ``yoperations``, non-linear spectra, MPI, one engine per output name, reading the reference's files, downloading a file.
"""
import numpy as np

from .. import _device as dv
from .. import utils
from ..cosmology import BaseEngine, BaseSection, BaseBackground, CosmologyError, find_conflicts, _conflict_parameters
from ..interpolator import Interpolator1D, PowerSpectrumInterpolator1D, PowerSpectrumInterpolator2D, _host
from . import get_default_z_callable


def _times(value, factor):
    """``value`` (device tensor or host array with the batch as leading axis) times ``factor`` (a float, or one host value per cosmology)."""
    if np.ndim(factor) == 0:
        factor = float(factor)
        return value if factor == 1. else value * factor
    if dv.is_torch(value):
        factor = dv.to_device(np.asarray(factor, dtype='f8'), value.device)
    else:
        factor = np.asarray(factor, dtype='f8')
    return value * factor.reshape(tuple(factor.shape) + (1,) * (np.ndim(value) - factor.ndim))


class EmulatedEngine(BaseEngine):

    """Engine using an emulator (reference emulated.py:36-175).  ``EmulatedEngine.read(filename)`` gives the engine class of one file, written by
    :meth:`Emulator.save`.

    Every parameter of the emulator is taken from the cosmology, ``self[name]``.  One the cosmology cannot provide raises :class:`CosmologyError`
    naming it (the reference skips it silently and lets the emulator fail later), but for the amplitude: an emulator that takes ``sigma8`` of a
    cosmology given ``A_s`` is handed the fiducial guess of sigma8, and the reverse, and the linear spectra are then rescaled by ``_rsigma8**2`` to the
    amplitude the cosmology states, as in the reference.  Here the same holds for an emulator that takes no amplitude at all (trained at a fixed one):
    its spectra are rescaled to the cosmology's ``sigma8``, or ``A_s``."""
    name = 'emulated'
    path = None

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        emulator = getattr(self.__class__, '_emulator', None)
        if emulator is None:
            if self.path is None:
                raise CosmologyError('no emulator file: use the engine class that EmulatedEngine.read(filename) returns')
            from . import Emulator
            emulator = Emulator.load(str(self.path), device=self.device)
            self.__class__._emulator = emulator      # loaded once per class, i.e. per call of read()
        self._A_s = self._get_A_s_fid()
        self._sigma8 = self._get_sigma8_fid()
        self._needs_rescale = None
        amplitudes = ('A_s',) + tuple(find_conflicts('A_s', conflicts=_conflict_parameters))      # 'A_s', 'logA', ..., 'sigma8'
        params = {}
        for name in emulator.params:
            try:
                params[name] = self[name]
            except CosmologyError:
                if name == 'sigma8':      # A_s provided by the cosmology, the emulator wants sigma8
                    params[name] = self._sigma8
                elif name == 'A_s':       # sigma8 provided by the cosmology, the emulator wants A_s
                    params[name] = self._A_s
                elif name in amplitudes:  # ... or its logarithm
                    params[name] = np.log(1e10 * self._A_s) if not dv.is_torch(self._A_s) else dv.torch().log(1e10 * self._A_s)
                else:
                    raise CosmologyError('Parameter {} of the emulator {} not found in the cosmology.'.format(name, self.path))
        if 'm_ncdm' in params:      # (reference :82-83)
            params['m_ncdm'] = self['m_ncdm_tot']
        # the emulator's spectra are at the amplitude it was handed, or trained at; the cosmology states its own as sigma8, or as A_s
        if 'sigma8' in self._params and 'sigma8' not in emulator.params:
            self._needs_rescale = 'sigma8'
        elif 'A_s' in self._params and not any(name in emulator.params for name in amplitudes if name != 'sigma8'):
            self._needs_rescale = 'A_s'
        self._emulator_params = params

    def _get_sigma8_fid(self):
        """First guess for sigma8 given A_s (reference cosmology.py:512-517)."""
        if 'sigma8' in self._params:
            return self._params['sigma8']
        return (self['A_s'] / 2.43e-9)**0.5 * 0.87659

    def _predict(self, section):
        """{name: value} of the emulator's outputs '<section>.<name>': varied ones as device tensors, with the batch as leading axis for a batch of
        cosmologies, fixed ones as they were saved.  One launch of the engine, on the columns of this section."""
        prefix = section + '.'
        emulator = self._emulator
        if not any(key.startswith(prefix) for key in list(emulator.varied_keys) + list(emulator.fixed)):
            raise CosmologyError('the emulator {} holds no {} quantity'.format(self.path, section))
        params = self._emulator_params
        if self.batch_size is not None:      # every cosmology of the batch, also if the emulator's own parameters are all scalars
            params = {name: value if np.ndim(value) else np.full(self.batch_size, value, dtype='f8') for name, value in params.items()}
        predict = emulator.predict(params, keys=section, device=True)
        return {key[len(prefix):]: value for key, value in predict.items()}

    @classmethod
    def read(cls, filename):
        """Return an engine subclass that will load ``filename`` (a file of :meth:`Emulator.save`) on first use, and keep the emulator.  The name
        'emulated' stays registered to the class it was: ``get_engine('emulated')`` is not the engine of the file read last."""
        from ..cosmology import RegisteredEngine
        registered = RegisteredEngine._registry.get(cls.name, None)

        class _EmulatedEngine(cls):

            path = filename
            __module__ = cls.__module__

        if registered is not None:
            RegisteredEngine._registry[cls.name] = registered
        return _EmulatedEngine

    @classmethod
    def load(cls, filename):
        """Deprecated. Use :meth:`read`."""
        import warnings
        warnings.warn('load() is deprecated, use read() instead.', DeprecationWarning, stacklevel=2)
        return cls.read(filename)

    def _rescale_sigma8(self):
        """Rescale perturbative quantities to match input sigma8 or A_s (reference emulated.py:144-175, linear spectra only): one host value, or one per
        cosmology of a batch."""
        if getattr(self, '_rsigma8', None) is not None:
            return self._rsigma8
        self._rsigma8 = 1.
        perturbative = ('primordial', 'fourier')      # background and thermodynamics know no amplitude
        if self._needs_rescale == 'sigma8':      # sigma8 provided by the cosmology
            rsigma8 = np.asarray(_host(self._params['sigma8']), dtype='f8') / np.asarray(_host(self.get_fourier().sigma8_m), dtype='f8')
        elif self._needs_rescale == 'A_s':       # A_s provided by the cosmology
            rsigma8 = (np.asarray(_host(self._params['A_s']), dtype='f8') / np.asarray(_host(self.get_primordial().A_s), dtype='f8'))**0.5
        else:
            return self._rsigma8
        self._sections = {name: section for name, section in self._sections.items() if name not in perturbative}      # filled with _rsigma8 = 1
        self._rsigma8 = float(rsigma8) if rsigma8.ndim == 0 else rsigma8
        return self._rsigma8


class _EmulatedSection(BaseSection):

    """A section whose state is what the emulator predicts for it; ``__getstate__`` gives it back under the calculator's keys."""
    _section = None
    _emulated = True

    def __init__(self, engine):
        super().__init__(engine)
        self.__setstate__(engine._predict(self._section))

    def _get(self, name):
        try:
            return self._state[name]
        except KeyError:
            raise CosmologyError('the emulator {} holds no {}.{}'.format(self._engine.path, self._section, name))


class Background(BaseBackground):

    """Background quantities (reference emulated.py:178-231): ``rho_ncdm``, ``p_ncdm``, ``rho_fld``, ``time`` and ``comoving_radial_distance`` are cubic
    splines (``Interpolator1D(z, values, k=3)``) through the emulated tables on ``get_default_z_callable('background')``, NaN outside that grid;
    everything else follows from the parameters (:class:`BaseBackground`).  A batch of cosmologies gives (B,) + z.shape."""
    _section = 'background'
    _emulated = True

    def __init__(self, engine):
        super().__init__(engine)
        self.__setstate__(engine._predict(self._section))

    _get = _EmulatedSection._get

    def _interp(self, name, z):
        interp = self._get(name)
        if interp is None:
            raise CosmologyError('the emulator {} holds no {}.{}'.format(self._engine.path, self._section, name))
        out = interp(z)      # z.shape + what follows the redshifts in the table: (B,), (N_ncdm,), (B, N_ncdm)
        nz, nlead = np.ndim(z), out.ndim - np.ndim(z)
        if not nlead:
            return out
        # the batch, then the redshifts; species first of all, as BaseBackground has them
        order = list(range(nz, nz + nlead)) + list(range(nz))
        if name.endswith('_ncdm'):
            order = order[nlead - 1:nlead] + order[:nlead - 1] + order[nlead:]
        return out.permute(*order) if dv.is_torch(out) else np.transpose(out, order)

    def rho_ncdm(self, z, species=None):
        """Comoving density of massive neutrinos, every species (N_ncdm,) + z.shape or one."""
        if not self._N_ncdm:
            return super().rho_ncdm(z, species=species)
        return self._interp('rho_ncdm', z)[species if species is not None else slice(None)]

    def p_ncdm(self, z, species=None):
        """Pressure of massive neutrinos."""
        if not self._N_ncdm:
            return super().p_ncdm(z, species=species)
        return self._interp('p_ncdm', z)[species if species is not None else slice(None)]

    def rho_fld(self, z):
        """Comoving density of the dark energy fluid."""
        return self._interp('rho_fld', z)

    def time(self, z):
        """Proper time (age of the universe at z), in Gyr."""
        return self._interp('time', z)

    def comoving_radial_distance(self, z):
        """Comoving radial distance, in Mpc/h."""
        return self._interp('comoving_radial_distance', z)

    def __getstate__(self):
        """The calculator's keys: the tables on the default redshifts (``get_calculator`` of an emulated cosmology returns the emulator's outputs)."""
        state = {'z': get_default_z_callable('background')}
        state.update(self._tables)
        return state

    def __setstate__(self, state):
        state = dict(state)
        z = _host(state.pop('z', get_default_z_callable('background')))
        self._tables, self._state = {}, {}
        for name, value in state.items():
            value = dv.to_device(value, self.device)
            self._tables[name] = value
            # (..., nz) -> the redshifts first; nothing to interpolate without species
            self._state[name] = Interpolator1D(z, value.movedim(-1, 0), k=3, interp_x='lin', interp_fun='lin', extrap=False, assume_sorted=True,
                                               device=self.device) if value.numel() else None


@utils.addproperty('rs_drag', 'z_drag', 'rs_star', 'z_star', 'YHe')
class Thermodynamics(_EmulatedSection):

    """``rs_drag``, ``z_drag``, ``rs_star``, ``z_star``, ``YHe``: those the emulator holds (reference emulated.py:234-254); the others raise
    :class:`CosmologyError`."""
    _section = 'thermodynamics'

    def __getattr__(self, name):
        if name in ('_rs_drag', '_z_drag', '_rs_star', '_z_star', '_YHe'):
            raise CosmologyError('the emulator {} holds no thermodynamics.{}'.format(self.__dict__['_engine'].path, name[1:]))
        raise AttributeError(name)

    def __getstate__(self):
        return {name: self.__dict__['_' + name] for name in ['rs_drag', 'z_drag', 'rs_star', 'z_star', 'YHe'] if '_' + name in self.__dict__}

    def __setstate__(self, state):
        for name, value in state.items():
            setattr(self, '_' + name, value)


@utils.addproperty('k_pivot', 'n_s', 'alpha_s', 'beta_s')
class Primordial(_EmulatedSection):

    """Primordial power spectrum (reference emulated.py:292-366): ``A_s`` from the emulator, the shape from the cosmology's n_s, alpha_s, beta_s, k_pivot."""
    _section = 'primordial'

    def __init__(self, engine):
        super().__init__(engine)
        self._n_s, self._alpha_s, self._beta_s = engine['n_s'], engine['alpha_s'], engine['beta_s']
        self._k_pivot = engine['k_pivot'] / self._h
        self._rsigma8 = engine._rescale_sigma8()

    @property
    def A_s(self):
        r"""Scalar amplitude of the primordial power spectrum at :math:`k_\mathrm{pivot}`, unitless."""
        return _times(self._get('A_s'), np.asarray(self._rsigma8)**2)

    @property
    def ln_1e10_A_s(self):
        r""":math:`\ln(10^{10}A_s)`, unitless."""
        A_s = self.A_s
        return dv.torch().log(1e10 * A_s) if dv.is_torch(A_s) else np.log(1e10 * A_s)

    def pk_k(self, k, mode='scalar'):
        r"""The primordial spectrum of curvature perturbations at ``k`` [h/Mpc], in (Mpc/h)^3 (reference emulated.py:316-342); (B,) + k.shape for a batch."""
        ['scalar'].index(mode)
        kh = np.asarray(_host(k), dtype='f8')

        def lead(value):      # one value, or one per cosmology against the wavenumbers
            value = np.asarray(_host(value), dtype='f8')
            return value.reshape(value.shape + (1,) * kh.ndim) if value.ndim else value

        h, A_s, k_pivot, n_s, alpha_s, beta_s = (lead(value) for value in (self._h, self.A_s, self._k_pivot, self._n_s, self._alpha_s, self._beta_s))
        lnkkp = np.log(kh / k_pivot)
        return h**3 * A_s * (kh / k_pivot)**(n_s - 1. + 1. / 2. * alpha_s * lnkkp + 1. / 6. * beta_s * lnkkp**2)

    def pk_interpolator(self, mode='scalar'):
        """:class:`PowerSpectrumInterpolator1D` of :meth:`pk_k`."""
        batch = self._engine.batch_size is not None
        return PowerSpectrumInterpolator1D.from_callable(pk_callable=lambda k: self.pk_k(k, mode=mode).T if batch else self.pk_k(k, mode=mode), device=self.device)

    def __getstate__(self):
        return {'A_s': self.A_s}

    def __setstate__(self, state):
        self._state = dict(state)


def _make_tuple(of, size=2):
    if isinstance(of, str):
        of = (of,)
    of = list(of)
    of = of + [of[0]] * (size - len(of))
    return tuple(sorted(of))


class Fourier(_EmulatedSection):

    """Linear power spectra (reference emulated.py:447-611): the emulated tables on (k, z), one per cosmology of a batch, times ``_rsigma8**2``."""
    _section = 'fourier'

    def __init__(self, engine):
        super().__init__(engine)
        self._rsigma8 = engine._rescale_sigma8()

    @property
    def sigma8_m(self):
        r"""Current r.m.s. of matter perturbations in a sphere of 8 Mpc/h, unitless."""
        if not hasattr(self, '_sigma8_m'):
            self._sigma8_m = self.sigma8_z(0., of='delta_m')
        return self._sigma8_m

    def sigma_rz(self, r, z, of='delta_m', **kwargs):
        r"""R.m.s. of `of` perturbations in spheres of :math:`r` Mpc/h."""
        return self.pk_interpolator(of=of, **kwargs).sigma_rz(r, z)

    def sigma8_z(self, z, of='delta_m'):
        r"""R.m.s. of `of` perturbations in spheres of 8 Mpc/h."""
        return self.sigma_rz(8., z, of=of)

    def table(self, non_linear=False, of='delta_m'):
        """k, z and the power spectrum table (nk, nz) -- (B, nk, nz) device tensor for a batch -- of the pair ``of``, in (Mpc/h)^3."""
        if non_linear:
            raise CosmologyError('non-linear spectra are not emulated')
        of = _make_tuple(of)
        try:
            pk = self._state['pk'][of]
        except KeyError:
            raise CosmologyError('the emulator {} holds no fourier.pk.{}.{}'.format(self._engine.path, *of))
        return _host(self._get('k')), _host(self._get('z')), _times(pk, np.asarray(self._rsigma8)**2)

    def pk_interpolator(self, non_linear=False, of='delta_m', **kwargs):
        """:class:`PowerSpectrumInterpolator2D` over the emulated table of the pair ``of`` (a batch of tables for a batch of cosmologies); ``kwargs``: its
        arguments."""
        ka, za, pka = self.table(non_linear=non_linear, of=of)
        kwargs.setdefault('device', self.device)
        return PowerSpectrumInterpolator2D(ka, za, pka, **kwargs)

    def pk_kz(self, k, z, non_linear=False, of='delta_m'):
        """Power spectrum at ``k`` [h/Mpc] and ``z``, in (Mpc/h)^3: (B,) + k.shape + z.shape."""
        return self.pk_interpolator(non_linear=non_linear, of=of)(k, z)

    def __getstate__(self):
        """The calculator's keys: 'k', 'z' and the tables 'pk.<of1>.<of2>' the emulator holds."""
        state = {'k': self._get('k'), 'z': self._get('z')}
        for of in self._state.get('pk', {}):
            state['pk.{}.{}'.format(*of)] = self.table(of=of)[2]
        return state

    def __setstate__(self, state):
        self._state = {}
        for keyname, value in state.items():
            if keyname.startswith('pk'):
                name, *keys = keyname.split('.')
                self._state.setdefault(name, {})[tuple(keys)] = value
            else:      # k, z
                self._state[keyname] = value

