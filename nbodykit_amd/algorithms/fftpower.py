"""
FFTPower — the headline algorithm (reference
nbodykit/algorithms/fftpower.py): auto/cross P(k) / P(k,mu) / P_ell(k)
of periodic-box sources.  Same construction flow as the reference
(:194-334): cast sources to meshes with dtype='f8', compensated=True
(:703-730), compute the compensated complex fields on the GPU, form
p3d = c1 conj(c2) V with the zero mode cleared (:91-143, the
``nbk_power3d_f64`` kernel), then project to (k, mu) / multipole bins
(:507-701) with the ``nbk_bin_power_f64`` kernel + a tiny host/allreduce
tail, and pack BinnedStatistic results.
"""
import logging

import numpy

from nbodykit_amd import CurrentMPIComm, hiplib
from nbodykit_amd.base.catalog import CatalogSourceBase
from nbodykit_amd.base.mesh import MeshSource
from nbodykit_amd.binned_statistic import BinnedStatistic
from nbodykit_amd.pm import ComplexField, RealField


class FFTBase(object):
    """Shared setup for periodic-box FFT algorithms (reference :12-143)."""

    def __init__(self, first, second, Nmesh, BoxSize):
        first = _cast_source(first, Nmesh=Nmesh, BoxSize=BoxSize)
        if second is not None:
            second = _cast_source(second, Nmesh=Nmesh, BoxSize=BoxSize)
        else:
            second = first

        self.first = first
        self.second = second
        self.comm = first.comm
        assert second.comm is first.comm, \
            "communicator mismatch between input sources"

        if not numpy.array_equal(first.attrs['BoxSize'],
                                 second.attrs['BoxSize']):
            raise ValueError("'BoxSize' mismatch between sources in "
                             "FFTPower")

        self.attrs = {}
        self.attrs['Nmesh'] = first.attrs['Nmesh'].copy()
        self.attrs['BoxSize'] = first.attrs['BoxSize'].copy()
        self.attrs.update(zip(['Lx', 'Ly', 'Lz'], self.attrs['BoxSize']))
        self.attrs.update({'volume': self.attrs['BoxSize'].prod()})

    def save(self, output):
        import json
        from nbodykit_amd.utils import JSONEncoder
        if self.comm.rank == 0:
            self.logger.info('measurement done; saving result to %s'
                             % output)
            with open(output, 'w') as ff:
                json.dump(self.__getstate__(), ff, cls=JSONEncoder)

    @classmethod
    @CurrentMPIComm.enable
    def load(cls, output, comm=None):
        import json
        from nbodykit_amd.utils import JSONDecoder
        if comm.rank == 0:
            with open(output, 'r') as ff:
                state = json.load(ff, cls=JSONDecoder)
        else:
            state = None
        state = comm.bcast(state)
        self = object.__new__(cls)
        self.__setstate__(state)
        self.comm = comm
        return self

    def _compute_3d_power(self, first, second):
        """p3d = c1 conj(c2), zero mode cleared (but still binned), x V
        (reference :91-143)."""
        attrs = {}
        attrs.update(self.attrs)

        c1 = first.compute(mode='complex', Nmesh=self.attrs['Nmesh'])
        if first is second:
            c2 = c1
        else:
            c2 = second.compute(mode='complex', Nmesh=self.attrs['Nmesh'])

        lib = hiplib.require()
        p3d = ComplexField(c1.pm)
        hiplib.check(lib.nbk_power3d_f64(
            hiplib.dptr(p3d.value), hiplib.dptr(c1.value),
            hiplib.dptr(c2.value), float(self.attrs['BoxSize'].prod()),
            hiplib.i64_arr(c1.dims), hiplib.i64_arr(c1.off), 1,
            hiplib.cur_stream()), 'nbk_power3d_f64')

        N1 = c1.attrs.get('N', 0)
        N2 = c2.attrs.get('N', 0)
        attrs.update({'N1': N1, 'N2': N2})

        Pshot = 0
        if self.first is self.second:
            if 'shotnoise' in c1.attrs:
                Pshot = c1.attrs['shotnoise']
        attrs['shotnoise'] = Pshot
        return p3d, attrs

    def _compute_complex_pair(self):
        """The complex fields computed WITHOUT the compensation action
        (the fused nbk_power_bin_f64 kernel applies compensation on the
        fly), plus the same attrs _compute_3d_power returns.  Only valid
        when _fuse_info accepted both meshes."""
        attrs = {}
        attrs.update(self.attrs)

        def _compute_raw(mesh):
            saved = mesh.compensated
            mesh.compensated = False
            try:
                return mesh.compute(mode='complex',
                                    Nmesh=self.attrs['Nmesh'])
            finally:
                mesh.compensated = saved

        c1 = _compute_raw(self.first)
        c2 = c1 if self.second is self.first else _compute_raw(self.second)

        attrs.update({'N1': c1.attrs.get('N', 0),
                      'N2': c2.attrs.get('N', 0)})
        Pshot = 0
        if self.first is self.second:
            if 'shotnoise' in c1.attrs:
                Pshot = c1.attrs['shotnoise']
        attrs['shotnoise'] = Pshot
        return c1, c2, attrs

    def _compute_deferred_x(self, mesh):
        """Pre-x-pass spectrum ``(tensor, n_inner, mesh_attrs)`` for the
        deferred-x fused FFT+binning path (nbk_fft_x_bin_f64): the z and
        y FFT passes (+ pencil transpose when distributed) run here, the
        final x pass runs inside the binning kernel.  Computed WITHOUT
        the compensation action (the kernel applies it on the fly —
        _fuse_info already certified compensation is the mesh's only
        action).  Collective: the fused-paint gates inside
        to_complex_field are rank-invariant and the fallback
        (to_real_field + r2c_defer_x) is taken by all ranks together."""
        from nbodykit_amd.pm import r2c_defer_x
        res = mesh.to_complex_field(_defer_x=True)
        if res is NotImplemented:
            # chunked-paint fallback: for an interlaced mesh
            # to_real_field returns the COMBINED mesh (the reference's
            # c2r round trip), so a single pre-x field with the
            # interlaced compensation is exactly right
            real = mesh.to_real_field(normalize=True)
            tensor, n_inner = r2c_defer_x(real)
            res = (tensor, None, n_inner, dict(real.attrs))
        tensor, tensor2, n_inner, mattrs = res
        attrs = {}
        attrs.update(self.attrs)
        attrs.update({'N1': mattrs.get('N', 0), 'N2': mattrs.get('N', 0)})
        attrs['shotnoise'] = mattrs.get('shotnoise', 0) \
            if self.first is self.second else 0
        return tensor, tensor2, n_inner, attrs


class FFTPower(FFTBase):
    """Periodic-box 1d/2d power spectrum and multipoles via FFT
    (reference :146-359; same signature and defaults)."""
    logger = logging.getLogger('FFTPower')

    def __init__(self, first, mode, Nmesh=None, BoxSize=None, second=None,
                 los=[0, 0, 1], Nmu=5, dk=None, kmin=0., kmax=None,
                 poles=[]):
        if mode not in ['1d', '2d']:
            raise ValueError("`mode` should be either '1d' or '2d'")
        if poles is None:
            poles = []

        if numpy.isscalar(los) or len(los) != 3:
            raise ValueError("line-of-sight ``los`` should be vector with "
                             "length 3")
        if not numpy.allclose(numpy.einsum('i,i', los, los), 1.0,
                              rtol=1e-5):
            raise ValueError("line-of-sight ``los`` must be a unit vector")

        FFTBase.__init__(self, first, second, Nmesh, BoxSize)

        self.attrs['mode'] = mode
        self.attrs['los'] = los
        self.attrs['Nmu'] = Nmu
        self.attrs['poles'] = poles

        if dk is None:
            dk = 2 * numpy.pi / self.attrs['BoxSize'].min()
        self.attrs['dk'] = dk
        self.attrs['kmin'] = kmin
        self.attrs['kmax'] = kmax

        self.power, self.poles = self.run()
        self.attrs.update(self.power.attrs)

    def run(self):
        if self.attrs['mode'] == '1d':
            self.attrs['Nmu'] = 1

        # the fused single-pass path: compensation + cross power + binning
        # in one kernel, p3d never materialized (nbk_power_bin_f64); falls
        # back to the explicit sequence for meshes with user actions
        fuse1 = _fuse_info(self.first)
        fuse2 = fuse1 if self.second is self.first \
            else _fuse_info(self.second)
        fused = fuse1 is not None and fuse2 is not None

        dk = self.attrs['dk']
        kmin = self.attrs['kmin']
        kmax = self.attrs['kmax']

        # deferred-x path (auto power, dk>0): the final x FFT pass runs
        # INSIDE the binning kernel (nbk_fft_x_bin_f64) — the finished
        # complex field is never materialized.  Edge arrays must be
        # known up front, so the dk == 0 unique-edges path stays on the
        # standard flow.
        defer = (fused and self.second is self.first and dk > 0
                 and kmin >= 0
                 and _xbin_ok(self.first, self.attrs['Nmesh']))
        if defer:
            kmax_eff = kmax
            if kmax_eff is None:
                kmax_eff = (numpy.pi * self.attrs['Nmesh'].min()
                            / self.attrs['BoxSize'].max() + dk / 2)
            kedges_d = numpy.arange(kmin, kmax_eff, dk)
            n0 = int(self.attrs['Nmesh'][0])
            poles_l = list(self.attrs['poles'])
            nell = len(poles_l) + (0 not in poles_l)
            defer = len(kedges_d) >= 1 and _xbin_lds_fits(
                n0, len(kedges_d), self.attrs['Nmu'] + 1, nell,
                il=bool(getattr(self.first, 'interlaced', False)))

        if defer:
            tensor, tensor2, n_inner, attrs = \
                self._compute_deferred_x(self.first)
            pm = self.first.pm
            Nmesh_arr = numpy.asarray(pm.Nmesh)
            BoxSize_arr = numpy.asarray(pm.BoxSize)
            y3d = None
        else:
            if fused:
                c1, c2, attrs = self._compute_complex_pair()
                y3d = c1     # coordinate/metadata source only
            else:
                y3d, attrs = self._compute_3d_power(self.first,
                                                    self.second)
            Nmesh_arr = y3d.Nmesh
            BoxSize_arr = y3d.BoxSize

        if kmax is None:
            kmax = numpy.pi * Nmesh_arr.min() / BoxSize_arr.max() + dk / 2

        if dk > 0:
            kedges = numpy.arange(kmin, kmax, dk)
            kcoords = None
        else:
            kedges, kcoords = _find_unique_edges(
                y3d.x, 2 * numpy.pi / y3d.BoxSize, kmax, y3d.pm.comm)

        muedges = numpy.linspace(-1, 1, self.attrs['Nmu'] + 1,
                                 endpoint=True)
        edges = [kedges, muedges]
        coords = [kcoords, None]
        if defer:
            result, pole_result = _project_power_xbin(
                tensor, tensor2, pm, n_inner, fuse1,
                volume=self.attrs['BoxSize'].prod(), edges=edges,
                poles=self.attrs['poles'], los=self.attrs['los'])
        elif fused:
            result, pole_result = _project_power_fused(
                c1, c2, fuse1, fuse2,
                volume=self.attrs['BoxSize'].prod(), edges=edges,
                poles=self.attrs['poles'], los=self.attrs['los'])
        else:
            result, pole_result = project_to_basis(
                y3d, edges, poles=self.attrs['poles'],
                los=self.attrs['los'])

        # pack the structured arrays (reference :306-334)
        if self.attrs['mode'] == '1d':
            cols = ['k', 'power', 'modes']
            icols = [0, 2, 3]
            edges = edges[0:1]
            coords = coords[0:1]
        else:
            cols = ['k', 'mu', 'power', 'modes']
            icols = [0, 1, 2, 3]

        dtype = numpy.dtype([(name, result[icol].dtype.str)
                             for icol, name in zip(icols, cols)])
        power = numpy.squeeze(numpy.empty(result[0].shape, dtype=dtype))
        for icol, col in zip(icols, cols):
            power[col][:] = numpy.squeeze(result[icol])

        poles = None
        if pole_result is not None:
            k, poles_arr, N = pole_result
            cols = ['k'] + ['power_%d' % l for l in self.attrs['poles']] \
                + ['modes']
            result = [k] + [pole for pole in poles_arr] + [N]
            dtype = numpy.dtype([(name, result[icol].dtype.str)
                                 for icol, name in enumerate(cols)])
            poles = numpy.empty(result[0].shape, dtype=dtype)
            for icol, col in enumerate(cols):
                poles[col][:] = result[icol]

        return self._make_datasets(edges, poles, power, coords, attrs)

    def __getstate__(self):
        return dict(power=self.power.__getstate__(),
                    poles=(self.poles.__getstate__()
                           if self.poles is not None else None),
                    attrs=self.attrs)

    def __setstate__(self, state):
        self.attrs = state['attrs']
        self.power = BinnedStatistic.from_state(state['power'])
        self.poles = None
        if state['poles'] is not None:
            self.poles = BinnedStatistic.from_state(state['poles'])

    def _make_datasets(self, edges, poles, power, coords, attrs):
        if self.attrs['mode'] == '1d':
            power = BinnedStatistic(['k'], edges, power,
                                    fields_to_sum=['modes'], coords=coords,
                                    **attrs)
        else:
            power = BinnedStatistic(['k', 'mu'], edges, power,
                                    fields_to_sum=['modes'], coords=coords,
                                    **attrs)
        if poles is not None:
            poles = BinnedStatistic(['k'], [power.edges['k']], poles,
                                    fields_to_sum=['modes'],
                                    coords=[power.coords['k']], **attrs)
        return power, poles


class ProjectedFFTPower(FFTBase):
    """Power spectrum of a field projected over axes (reference
    fftpower.py:361-505).  Following the reference, the projected FFT
    runs on the gathered preview with numpy.fft.rfftn — that is the
    reference's own host-side path (:443), not a GPU fallback; the
    painting/compensation still runs on the GPU."""
    logger = logging.getLogger('ProjectedFFTPower')

    def __init__(self, first, Nmesh=None, BoxSize=None, second=None,
                 axes=(0, 1), dk=None, kmin=0.):
        FFTBase.__init__(self, first, second, Nmesh, BoxSize)

        assert len(axes) in (1, 2),             "length of ``axes`` in ProjectedFFTPower should be 1 or 2"

        if dk is None:
            dk = 2 * numpy.pi / self.attrs['BoxSize'].min()
        self.attrs['dk'] = dk
        self.attrs['kmin'] = kmin
        self.attrs['axes'] = list(axes)
        self.run()

    def run(self):
        axes = self.attrs['axes']
        c1 = self.first.compute(Nmesh=self.attrs['Nmesh'], mode='real')
        r1 = c1.preview(self.attrs['Nmesh'], axes=axes)
        c1 = numpy.fft.rfftn(r1) / self.attrs['Nmesh'].prod()  # :443

        if self.first is self.second:
            c2 = c1
        else:
            c2f = self.second.compute(Nmesh=self.attrs['Nmesh'],
                                      mode='real')
            r2 = c2f.preview(self.attrs['Nmesh'], axes=axes)
            c2 = numpy.fft.rfftn(r2) / self.attrs['Nmesh'].prod()

        pk = c1 * c2.conj()
        pk.flat[0] = 0    # zero mode

        shape = numpy.array([self.attrs['Nmesh'][i] for i in axes],
                            dtype='int')
        boxsize = numpy.array([self.attrs['BoxSize'][i] for i in axes])
        I = numpy.eye(len(shape), dtype='int') * -2 + 1

        k = [numpy.fft.fftfreq(N, 1. / (N * 2 * numpy.pi / L))[:pkshape]
             .reshape(kshape)
             for N, L, kshape, pkshape in zip(shape, boxsize, I, pk.shape)]

        kmag = sum(ki ** 2 for ki in k) ** 0.5
        W = numpy.empty(pk.shape, dtype='f4')
        W[...] = 2.0
        W[..., 0] = 1.0
        W[..., -1] = 1.0

        dk = self.attrs['dk']
        kmin = self.attrs['kmin']
        kedges = numpy.arange(
            kmin,
            numpy.pi * self.attrs['Nmesh'][axes].min()
            / self.attrs['BoxSize'][axes].max() + dk / 2, dk)

        xsum = numpy.zeros(len(kedges) + 1)
        Psum = numpy.zeros(len(kedges) + 1, dtype='complex128')
        Nsum = numpy.zeros(len(kedges) + 1)

        dig = numpy.digitize(kmag.flat, kedges)
        xsum.flat += numpy.bincount(dig, weights=(W * kmag).flat,
                                    minlength=xsum.size)
        Psum.real.flat += numpy.bincount(dig, weights=(W * pk.real).flat,
                                         minlength=xsum.size)
        Psum.imag.flat += numpy.bincount(dig, weights=(W * pk.imag).flat,
                                         minlength=xsum.size)
        Nsum.flat += numpy.bincount(dig, weights=W.flat,
                                    minlength=xsum.size)

        self.power = numpy.empty(len(kedges) - 1,
                                 dtype=[('k', 'f8'), ('power', 'c16'),
                                        ('modes', 'f8')])
        with numpy.errstate(invalid='ignore', divide='ignore'):
            self.power['k'] = (xsum / Nsum)[1:-1]
            self.power['power'] = (Psum / Nsum)[1:-1] * boxsize.prod()
            self.power['modes'] = Nsum[1:-1]

        self.edges = kedges
        self.power = BinnedStatistic(['k'], [self.edges], self.power)

    def __getstate__(self):
        return dict(edges=self.edges, power=self.power.data,
                    attrs=self.attrs)

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.power = BinnedStatistic(['k'], [self.edges], self.power)


def project_to_basis(y3d, edges, los=[0, 0, 1], poles=[]):
    """
    Project a 3D statistic (ComplexField in k-space, or RealField in
    configuration space — the FFTCorr case) onto (x, mu) bins and
    multipoles (reference :507-701), with the sums done by the
    ``nbk_bin_power_f64`` HIP kernel and the tiny fold/normalize tail on
    host after one small allreduce (the reference's :669-679).
    """
    import torch
    comm = y3d.pm.comm
    lib = hiplib.require()
    real_field = isinstance(y3d, RealField)

    xedges, muedges = edges
    Nx = len(xedges) - 1
    Nmu = len(muedges) - 1

    poles = list(poles)
    do_poles = len(poles) > 0
    _poles = [0] + sorted(poles) if 0 not in poles else sorted(poles)
    ell_idx = [_poles.index(l) for l in poles]
    Nell = len(_poles)
    if any(ell < 0 for ell in _poles):
        raise ValueError("in `project_to_basis`, multipole numbers must be "
                         "non-negative integers")

    NB = (Nx + 2) * (Nmu + 2)
    nfields = 3 + 2 * Nell

    dev = 'cuda'
    k2edges_t = torch.as_tensor(numpy.asarray(xedges, dtype='f8') ** 2) \
        .to(dev)
    muedges_t = torch.as_tensor(numpy.asarray(muedges, dtype='f8')).to(dev)
    sums = torch.zeros(nfields * NB, dtype=torch.float64, device=dev)

    if real_field:
        dims = tuple(int(d) for d in y3d.value.shape)
        off = (y3d.x_start, 0, 0)
    else:
        dims = y3d.dims
        off = y3d.off

    hiplib.check(lib.nbk_bin_power_f64(
        hiplib.dptr(y3d.value), hiplib.i64_arr(y3d.pm.Nmesh),
        hiplib.f64_arr(y3d.pm.BoxSize),
        hiplib.i64_arr(dims), hiplib.i64_arr(off), None,
        hiplib.dptr(k2edges_t), len(xedges),
        hiplib.dptr(muedges_t), len(muedges),
        hiplib.f64_arr(los), hiplib.int_arr(_poles), Nell,
        int(real_field),
        hiplib.dptr(sums), hiplib.dptr(sums[NB:]),
        hiplib.dptr(sums[2 * NB:]), hiplib.dptr(sums[3 * NB:]),
        hiplib.cur_stream()), 'nbk_bin_power_f64')

    torch.cuda.synchronize()
    host = sums.cpu().numpy()
    host = comm.allreduce(host)
    return _fold_bin_sums(host, Nx, Nmu, Nell, ell_idx, do_poles,
                          real_field)


def _fold_bin_sums(host, Nx, Nmu, Nell, ell_idx, do_poles, real_field):
    """Host tail of project_to_basis: unpack the kernel's planar sums,
    fold the internal mu == 1 bin, normalize (fftpower.py:669-701)."""
    NB = (Nx + 2) * (Nmu + 2)
    shape = (Nx + 2, Nmu + 2)
    xsum = host[:NB].reshape(shape)
    musum = host[NB:2 * NB].reshape(shape)
    Nsum = numpy.round(host[2 * NB:3 * NB]).astype('i8').reshape(shape)
    # kernel layout is planar: [y0.re | y0.im | y1.re | ...] (NB each)
    ys = host[3 * NB:].reshape(Nell, 2, NB)
    if real_field:
        # real statistic: ysum carries no imaginary part
        # (reference ysum dtype follows y3d.dtype, fftpower.py:597)
        ysum = ys[:, 0].reshape((Nell,) + shape).copy()
    else:
        ysum = (ys[:, 0] + 1j * ys[:, 1]).reshape((Nell,) + shape)

    # fold the internal mu == 1 bin into the last visible bin (:674-679)
    ysum[..., -2] += ysum[..., -1]
    musum[:, -2] += musum[:, -1]
    xsum[:, -2] += xsum[:, -1]
    Nsum[:, -2] += Nsum[:, -1]

    sl = slice(1, -1)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        y2d = (ysum[0] / Nsum)[sl, sl]
        xmean_2d = (xsum / Nsum)[sl, sl]
        mumean_2d = (musum / Nsum)[sl, sl]
        N_2d = Nsum[sl, sl]

        if do_poles:
            N_1d = Nsum[sl, sl].sum(axis=-1)
            xmean_1d = xsum[sl, sl].sum(axis=-1) / N_1d
            pole_arr = ysum[:, sl, sl].sum(axis=-1) / N_1d
            pole_arr = pole_arr[ell_idx, ...]
            pole_result = (xmean_1d, pole_arr, N_1d)
        else:
            pole_result = None

    return (xmean_2d, mumean_2d, y2d, N_2d), pole_result


def _fuse_info(mesh):
    """(window_id, interlaced) for the fused compensate+power+bin kernel,
    or None when the mesh cannot take the fused path.  Fusable: a plain
    CatalogMesh with no user actions, whose only k-space work is the
    auto-prepended compensation (source/mesh/catalog.py:405-451);
    window -1 encodes compensated=False."""
    from nbodykit_amd.base.mesh import MeshSource
    from nbodykit_amd.source.mesh.catalog import (CatalogMesh,
                                                  lookup_compensation)
    if not isinstance(mesh, CatalogMesh):
        return None
    if len(MeshSource.actions.fget(mesh)) != 0:
        return None
    if not mesh.compensated:
        return (-1, 0)
    try:
        actions = mesh._get_compensation()
    except ValueError:
        return None
    comp = lookup_compensation(actions[0][1])
    if comp is None:
        return None
    window, interlaced = comp
    return (hiplib.WINDOW_IDS[window], int(interlaced))


def _project_power_fused(c1, c2, comp1, comp2, volume, edges,
                         los=[0, 0, 1], poles=[]):
    """project_to_basis of comp1(c1) conj(comp2(c2)) V with the zero mode
    cleared, in ONE streaming pass over the complex field(s)
    (nbk_power_bin_f64) — the compensate/power3d/bin sequence without
    materializing p3d.  Bin assignment is bit-identical to the unfused
    path (same k2/mu operation grouping); values agree to roundoff —
    the fast kernel composes the separable compensation as per-axis
    reciprocal products where nbk_compensate_f64 chains divides, a
    last-ulp difference pinned by test_fused_power_matches_unfused at
    1e-10."""
    import torch
    comm = c1.pm.comm
    lib = hiplib.require()

    xedges, muedges = edges
    Nx = len(xedges) - 1
    Nmu = len(muedges) - 1

    poles = list(poles)
    do_poles = len(poles) > 0
    _poles = [0] + sorted(poles) if 0 not in poles else sorted(poles)
    ell_idx = [_poles.index(l) for l in poles]
    Nell = len(_poles)
    if any(ell < 0 for ell in _poles):
        raise ValueError("in `project_to_basis`, multipole numbers must "
                         "be non-negative integers")

    NB = (Nx + 2) * (Nmu + 2)
    nfields = 3 + 2 * Nell

    dev = 'cuda'
    k2edges_t = torch.as_tensor(numpy.asarray(xedges, dtype='f8') ** 2) \
        .to(dev)
    muedges_t = torch.as_tensor(numpy.asarray(muedges, dtype='f8')).to(dev)
    sums = torch.zeros(nfields * NB, dtype=torch.float64, device=dev)

    win1, interl1 = comp1
    win2, interl2 = comp2
    hiplib.check(lib.nbk_power_bin_f64(
        hiplib.dptr(c1.value), hiplib.dptr(c2.value), float(volume),
        int(win1), int(interl1), int(win2), int(interl2), 1,
        hiplib.i64_arr(c1.pm.Nmesh), hiplib.f64_arr(c1.pm.BoxSize),
        hiplib.i64_arr(c1.dims), hiplib.i64_arr(c1.off), None,
        hiplib.dptr(k2edges_t), len(xedges),
        hiplib.dptr(muedges_t), len(muedges),
        hiplib.f64_arr(los), hiplib.int_arr(_poles), Nell,
        hiplib.dptr(sums), hiplib.dptr(sums[NB:]),
        hiplib.dptr(sums[2 * NB:]), hiplib.dptr(sums[3 * NB:]),
        hiplib.cur_stream()), 'nbk_power_bin_f64')

    torch.cuda.synchronize()
    host = sums.cpu().numpy()
    host = comm.allreduce(host)
    return _fold_bin_sums(host, Nx, Nmu, Nell, ell_idx, do_poles,
                          real_field=False)


def _xbin_ok(mesh, Nmesh):
    """True when the deferred-x fused FFT+binning kernel can serve this
    mesh: non-interlaced, already at the target Nmesh (no spectral
    resample), power-of-two axes in [8, 4096] (the in-LDS x-line FFT),
    and not disabled via NBK_NO_XBIN=1.  Every term is rank-invariant,
    so the decision is collective."""
    import os
    if os.environ.get('NBK_NO_XBIN', '0') == '1':
        return False
    pmN = numpy.asarray(mesh.pm.Nmesh)
    if not numpy.array_equal(pmN, numpy.asarray(Nmesh)):
        return False
    for n in pmN:
        n = int(n)
        if n < 8 or n > 4096 or (n & (n - 1)):
            return False
    return True


def _xbin_lds_fits(n0, nx_edges, nmu_edges, nell, il=False):
    """Mirror of nbk_fft_x_bin_f64's LDS budget: histograms + edge
    arrays + compensation (+ interlace phase) tables + the TI=1 FFT
    tile(s) must fit the gfx950 160 KiB LDS less the 4 KiB the launcher
    reserves for the kernel's static arrays, and the register pipeline
    caps n0*TI (the kernel itself would return NBK_ERR_UNSUPPORTED;
    gate here so the standard path is taken without a failed
    launch)."""
    NB = (nx_edges + 1) * (nmu_edges + 1)
    fixed = (NB * (3 + 2 * nell) + nx_edges + nmu_edges + n0) * 8
    if il:
        fixed += n0 * 16                       # x phase table
        if n0 > 2048:
            return False
    nbufs = 2 if il else 1
    # the kernel's static arrays share the 160 KiB (NBK_XBIN_STATIC_LDS)
    budget = 160 * 1024 - 4096
    return fixed + nbufs * n0 * 2 * 16 <= budget      # TI=1, pitch 2


def _project_power_xbin(tensor, tensor2, pm, n_inner, comp1, volume,
                        edges, los=[0, 0, 1], poles=[]):
    """project_to_basis of |comp1(F_x(pre_x))|^2 V with the zero mode
    cleared, fused into the final x-axis FFT pass (nbk_fft_x_bin_f64):
    the finished complex field never exists in HBM and columns wholly
    beyond the last k-edge are skipped before their loads.  Auto power
    only.  Bin assignment is bit-identical to the unfused path (same
    k2/mu groupings); the x-FFT element values are bit-identical to
    nbk_fft_c_strided's.

    ``tensor2`` (interlaced meshes): the half-cell-shifted paint's
    pre-x field — the kernel combines the pair per element; the two
    self-conjugate z planes (whose Hermitian projection couples
    columns) are skipped there and handled here with the standalone
    kernels, accumulating into the same sums buffer."""
    import torch
    comm = pm.comm
    ws = comm.size
    lib = hiplib.require()

    xedges, muedges = edges
    Nx = len(xedges) - 1
    Nmu = len(muedges) - 1

    poles = list(poles)
    do_poles = len(poles) > 0
    _poles = [0] + sorted(poles) if 0 not in poles else sorted(poles)
    ell_idx = [_poles.index(l) for l in poles]
    Nell = len(_poles)
    if any(ell < 0 for ell in _poles):
        raise ValueError("in `project_to_basis`, multipole numbers must "
                         "be non-negative integers")

    NB = (Nx + 2) * (Nmu + 2)
    nfields = 3 + 2 * Nell

    dev = 'cuda'
    k2edges_t = torch.as_tensor(numpy.asarray(xedges, dtype='f8') ** 2) \
        .to(dev)
    muedges_t = torch.as_tensor(numpy.asarray(muedges, dtype='f8')).to(dev)
    sums = torch.zeros(nfields * NB, dtype=torch.float64, device=dev)

    win1, interl1 = comp1
    y_off = pm.y_start if ws > 1 else 0
    # uniform-grid digitize guesses (run() gated on dk > 0, kmin >= 0;
    # the kernel corrects the guess against the exact edges, so these
    # never change the assignment)
    dk_g = float(xedges[1] - xedges[0]) if Nx >= 1 else 1.0
    dmu_g = float(muedges[1] - muedges[0]) if Nmu >= 1 else 1.0
    hints = hiplib.f64_arr([float(xedges[0]), 1.0 / dk_g,
                            float(muedges[0]), 1.0 / dmu_g])
    hiplib.check(lib.nbk_fft_x_bin_f64(
        hiplib.dptr(tensor),
        hiplib.dptr(tensor2) if tensor2 is not None else None,
        hiplib.i64_arr(pm.Nmesh),
        int(n_inner), int(y_off), hiplib.f64_arr(pm.BoxSize),
        int(win1), int(interl1), 1, float(volume),
        hiplib.dptr(k2edges_t), len(xedges),
        hiplib.dptr(muedges_t), len(muedges), hints,
        hiplib.f64_arr(los), hiplib.int_arr(_poles), Nell,
        hiplib.dptr(sums), hiplib.cur_stream()), 'nbk_fft_x_bin_f64')

    if tensor2 is not None:
        _xbin_conj_planes(tensor, tensor2, pm, n_inner, y_off, comp1,
                          volume, k2edges_t, xedges, muedges_t, muedges,
                          los, _poles, Nell, NB, sums)

    torch.cuda.synchronize()
    host = sums.cpu().numpy()
    host = comm.allreduce(host)
    return _fold_bin_sums(host, Nx, Nmu, Nell, ell_idx, do_poles,
                          real_field=False)


def _xbin_conj_planes(tensor, tensor2, pm, n_inner, y_off, comp1,
                      volume, k2edges_t, xedges, muedges_t, muedges,
                      los, _poles, Nell, NB, sums):
    """The interlaced pair's self-conjugate z planes (kz = 0 and, for
    even n2, the Nyquist plane): x-FFT both paints' plane slices,
    combine with exp(i k.H/2), apply the Hermitian projection
    c <- (c + conj(c(-k)))/2 over the (kx, ky) mirror — allgathered
    when y is partitioned — and bin with the standalone fused kernel
    (source/mesh/catalog.py applies the same projection on the
    materialized field; the reference gets it from the c2r + re-r2c
    round trip)."""
    import torch
    from nbodykit_amd.pm import fft_axis1, all_gather_tensor, _int_freqs
    lib = hiplib.require()
    comm = pm.comm
    ws = comm.size
    s = hiplib.cur_stream()
    n0, n1, n2 = (int(x) for x in pm.Nmesh)
    nzh = n2 // 2 + 1
    nyl = int(n_inner) // nzh
    win1, interl1 = comp1

    planes = [0] + ([n2 // 2] if n2 % 2 == 0 else [])
    fxt = torch.as_tensor(_int_freqs(n0)).to('cuda')
    fyt = torch.as_tensor(_int_freqs(n1)[y_off:y_off + nyl]).to('cuda')
    for iz in planes:
        fz = float(iz) if iz == 0 else -float(n2 // 2)
        A = tensor.view(n0, -1)[:, iz::nzh].contiguous()
        B = tensor2.view(n0, -1)[:, iz::nzh].contiguous()
        fft_axis1(A.view(1, n0, nyl), -1, s)
        fft_axis1(B.view(1, n0, nyl), -1, s)
        # phase computed ON DEVICE (a host numpy exp of the full plane
        # cost ~4 ms/step at 512^3)
        ang = numpy.pi * (fxt[:, None] / n0 + fyt[None, :] / n1
                          + fz / n2)
        ph = torch.polar(torch.ones_like(ang), ang)
        C = 0.5 * A + 0.5 * B * ph
        if ws > 1:
            parts = [torch.empty_like(C) for _ in range(ws)]
            all_gather_tensor(parts, C.contiguous())
            Cf = torch.cat(parts, dim=1)
            M = torch.conj(torch.roll(torch.flip(Cf, (0, 1)),
                                      (1, 1), (0, 1)))
            C = (0.5 * (Cf + M))[:, y_off:y_off + nyl]
        else:
            M = torch.conj(torch.roll(torch.flip(C, (0, 1)),
                                      (1, 1), (0, 1)))
            C = 0.5 * (C + M)
        C = C.reshape(n0, nyl, 1).contiguous()
        hiplib.check(lib.nbk_power_bin_f64(
            hiplib.dptr(C), None, float(volume),
            int(win1), int(interl1), int(win1), int(interl1), 1,
            hiplib.i64_arr(pm.Nmesh), hiplib.f64_arr(pm.BoxSize),
            hiplib.i64_arr([n0, nyl, 1]),
            hiplib.i64_arr([0, y_off, iz]), None,
            hiplib.dptr(k2edges_t), len(xedges),
            hiplib.dptr(muedges_t), len(muedges),
            hiplib.f64_arr(los), hiplib.int_arr(_poles), Nell,
            hiplib.dptr(sums), hiplib.dptr(sums[NB:]),
            hiplib.dptr(sums[2 * NB:]), hiplib.dptr(sums[3 * NB:]),
            hiplib.cur_stream()), 'nbk_power_bin_f64')


def _cast_source(source, BoxSize, Nmesh):
    """Cast to a MeshSource; catalogs get dtype='f8', compensated=True
    (reference :703-730)."""
    from nbodykit_amd.source.mesh import FieldMesh

    if isinstance(source, (RealField, ComplexField)):
        source = FieldMesh(source)
    elif isinstance(source, CatalogSourceBase):
        if not isinstance(source, MeshSource):
            source = source.to_mesh(BoxSize=BoxSize, Nmesh=Nmesh,
                                    dtype='f8', compensated=True)

    if not isinstance(source, MeshSource):
        raise TypeError("Unknown type of source in FFTPower: %s"
                        % str(type(source)))
    if BoxSize is not None and any(source.attrs['BoxSize'] != BoxSize):
        raise ValueError("Mismatched Boxsize between __init__ and source.attrs")
    if Nmesh is not None and any(source.attrs['Nmesh'] != Nmesh):
        raise ValueError("Mismatched Nmesh between __init__ and "
                         "source.attrs; if trying to re-sample with a "
                         "different mesh, specify `Nmesh` as keyword of "
                         "to_mesh()")
    return source


def _find_unique_edges(x, x0, xmax, comm):
    """dk=0 unique-modulus edges (reference :732-769)."""
    fx2 = 0
    for xi in x:
        fx2 = fx2 + xi ** 2

    def find_unique_local(fx2, binning):
        fx2 = numpy.ravel(fx2)
        ix2 = numpy.int64(fx2 / binning + 0.5)
        ix2, ind = numpy.unique(ix2, return_index=True)
        return fx2[ind]

    binning = (x0.min() * 0.05) ** 2
    fx = find_unique_local(fx2, binning) ** 0.5
    fx = fx[fx < xmax]
    fx = numpy.concatenate(comm.allgather(fx), axis=0)
    minx0 = comm.allreduce(x0.min(), op='min')
    fx = find_unique_local(fx, minx0 * 1e-5)

    width = numpy.diff(fx)
    edges = fx.copy()
    edges[1:] -= width * 0.5
    edges = numpy.append(edges, [fx[-1] + width[-1] * 0.5])
    edges[0] = 0
    return edges, fx
