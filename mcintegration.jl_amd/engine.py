"""Engine: one mci_problem on one GPU (device-resident grids, histograms, statistics)."""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import LeafDesc, ProblemDesc, c_double_p, c_int32_p, check, lib
from .integrand import HostIntegrand, HostMeasure, Integrand, Measure
from .variables import ContinuousVar, FermiK

_ctx_cache = {}


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def context(device=0):
    """One mci_ctx (HIP stream + optional RCCL communicator) per device per process.
    device < 0 gives the offline, compile-only context (kernel cache pre-fill; no GPU needed)."""
    if device not in _ctx_cache:
        p = C.c_void_p()
        check(lib().mci_ctx_create(device, C.byref(p)))
        _ctx_cache[device] = p
    return _ctx_cache[device]


_live_engines = weakref.WeakSet()


def shutdown():
    """Close every live engine, then destroy every cached context (stream + RCCL communicator): the counterpart of
    MPI.Finalize.  Registered with atexit, so that device memory, streams and communicators are released while the HIP
    runtime and RCCL are still fully alive -- objects that survive into the interpreter's teardown are destroyed in an
    order nobody controls (seen: glibc "double free or corruption" at process exit, after all work had finished)."""
    for eng in list(_live_engines):
        try:
            eng.close()
        except Exception:
            pass
    for dev in list(_ctx_cache):
        try:
            lib().mci_ctx_destroy(_ctx_cache.pop(dev))
        except Exception:
            pass


atexit.register(shutdown)


def device_count():
    n = C.c_int32()
    lib().mci_device_count(C.byref(n))
    return n.value


class _HostObs(np.ndarray):
    """an observable handed to a host `measure` closure with a batch of records: `obs[i][bins] += w` with an integer ARRAY of bins
    (`obs[1][bin[1]] += weights[1]` of docs/src/index.md "Measure Histogram" over the records of a block) adds every record's weight to
    its bin -- numpy's own fancy `+=` would keep one of the records that share a bin.  An observable only accumulates
    (vegas/montecarlo.jl:156-161), so reading bins through an integer array gives zeros and storing through one adds."""

    def __new__(cls, n, dtype=float):
        return np.zeros(n, dtype=dtype).view(cls)

    @staticmethod
    def _bins(i):
        one = lambda q: isinstance(q, np.ndarray) and q.dtype.kind in "iu" and q.ndim >= 1
        return one(i) or (isinstance(i, tuple) and any(one(q) for q in i) and all(one(q) or isinstance(q, (int, np.integer)) for q in i))

    def __getitem__(self, i):
        if self._bins(i):
            return np.zeros(np.broadcast(*i).shape if isinstance(i, tuple) else i.shape, dtype=self.dtype)
        out = np.ndarray.__getitem__(self, i)
        return out.view(np.ndarray) if isinstance(out, np.ndarray) else out

    def __setitem__(self, i, v):
        if self._bins(i):
            np.add.at(self.view(np.ndarray), i, v)
            return
        np.ndarray.__setitem__(self, i, v)


def _slow_path_warning(what, unit, err):
    """said once per callback: a host closure that cannot take a batch is called per %(unit)s by the interpreter -- orders of magnitude
    below the traced path (integrate(..., trace=True) says why a closure was not traced)"""
    import warnings
    warnings.warn("the host %s closure raised on a batch of %ss (%s: %s) and is now called %s by %s: correct, but slow -- write it for "
                  "arrays, or make it traceable (integrate(..., trace=True) names what stops the tracer)"
                  % (what, unit, type(err).__name__, str(err)[:80], unit, unit), RuntimeWarning, stacklevel=2)


def _store_obs(O, obs, obs_nbin, nc):
    off = 0
    for o, nb in zip(obs, obs_nbin):
        o = np.asarray(o).reshape(-1)
        if nc == 2:
            O[off:off + nb:2], O[off + 1:off + nb:2] = o.real, o.imag
        else:
            O[off:off + nb] = o
        off += nb


class Engine:
    def __init__(self, config, integrand, measure=None, device=0, threads=None, wg_per_block=None, rng_bits=None, rng_rounds=None,
                 deterministic=False):
        L = lib()
        self.config = config
        self.device = device
        self.ctx = context(device)
        _live_engines.add(self)
        if isinstance(integrand, str):
            integrand = Integrand(integrand, config.userdata)
        elif callable(integrand) and not isinstance(integrand, (Integrand, HostIntegrand)):
            integrand = HostIntegrand(integrand)
        self.integrand = integrand
        if callable(measure) and not isinstance(measure, (Measure, HostMeasure)) and not hasattr(measure, "pool"):
            measure = HostMeasure(measure)   # a Python closure: host batch-callback path
        self.measure = measure               # None (the default measure), bin_by, Measure (device source) or HostMeasure
        leaves = config.leaves
        self._keep = []
        arr = (LeafDesc * len(leaves))()
        for i, lf in enumerate(leaves):
            d = arr[i]
            d.pool = config.leaf_pool[i]
            d.alpha, d.adapt = lf.alpha, 1 if lf.adapt else 0
            d.lower, d.upper = float(lf.lower), float(lf.upper)
            init = None
            # a variable that already lives in another, still open engine brings what it has learned there:
            # `integrate(...; var = (res.config.var[1], ...))` continues from the trained map (docs/src/index.md:129)
            prev = getattr(lf, "_engine", None)
            trained = prev is not None and prev is not self and getattr(prev, "p", None)
            if isinstance(lf, ContinuousVar):
                d.kind, d.npoints = _lib.CONTINUOUS, lf.ninc
                init = lf.grid if trained else lf._grid0
            elif isinstance(lf, FermiK):
                d.kind, d.npoints = _lib.FERMIK, lf.dim   # lower = kF, upper = dk, alpha = maxK
            else:
                d.kind, d.npoints = _lib.DISCRETE, 0
                init = lf.distribution if trained else lf._dist0
            if init is not None:
                init = np.ascontiguousarray(init, dtype=np.float64)
                self._keep.append(init)
                d.init = _dp(init)
        dof = np.ascontiguousarray(config.dof, dtype=np.int32)
        onb = np.ascontiguousarray(config.obs_nbin, dtype=np.int32)
        obd = np.ascontiguousarray(config.obs_bin_draw(measure), dtype=np.int32)
        nb_off = nb_list = None
        nbrs = config.neighbor_lists()   # None = the reference default (configuration.jl:203-208)
        if nbrs is not None:
            off = np.zeros(len(nbrs) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(n) for n in nbrs])
            flat = np.ascontiguousarray([j for n in nbrs for j in n], dtype=np.int32)
            self._keep += [off, flat]
            nb_off, nb_list = off.ctypes.data_as(c_int32_p), flat.ctypes.data_as(c_int32_p)
        desc = ProblemDesc(len(leaves), arr, len(config.var), config.N, dof.ctypes.data_as(c_int32_p),
                           onb.ctypes.data_as(c_int32_p), obd.ctypes.data_as(c_int32_p), nb_off, nb_list, config.ncomp)
        self.p = C.c_void_p()
        check(L.mci_problem_create(self.ctx, C.byref(desc), C.byref(self.p)))
        ud = integrand.userdata
        if isinstance(integrand, HostIntegrand) and getattr(integrand, "indexed", False):
            self._host_cb = _lib.HOST_INTEGRAND_IDX_FN(self._make_host_indexed_callback(integrand.fn))   # keep alive
            check(L.mci_set_integrand_host_indexed(self.p, C.cast(self._host_cb, C.c_void_p), None))
        elif isinstance(integrand, HostIntegrand):
            self._host_cb = _lib.HOST_INTEGRAND_FN(self._make_host_callback(integrand.fn, getattr(integrand, "inplace", False)))   # keep alive
            check(L.mci_set_integrand_host(self.p, C.cast(self._host_cb, C.c_void_p), None))
        else:
            check(L.mci_set_integrand_source(self.p, integrand.body.encode(), _dp(ud) if len(ud) else None, len(ud)))
        if isinstance(measure, Measure):
            check(L.mci_set_measure_source(self.p, measure.body.encode()))
        elif isinstance(measure, HostMeasure) and measure.indexed:
            self._host_measure_cb = _lib.HOST_MEASURE_IDX_FN(self._make_host_measure_indexed_callback(measure.fn))   # keep alive
            check(L.mci_set_measure_host_indexed(self.p, C.cast(self._host_measure_cb, C.c_void_p), None))
        elif isinstance(measure, HostMeasure):
            self._host_measure_cb = _lib.HOST_MEASURE_FN(self._make_host_measure_callback(measure.fn))   # keep alive
            check(L.mci_set_measure_host(self.p, C.cast(self._host_measure_cb, C.c_void_p), None))
        if threads or wg_per_block is not None:
            check(L.mci_set_launch(self.p, threads or 0, -1 if wg_per_block is None else wg_per_block))
        if rng_bits is not None:
            check(L.mci_set_rng_bits(self.p, int(rng_bits)))
        if rng_rounds is not None:
            check(L.mci_set_rng_rounds(self.p, int(rng_rounds)))
        if deterministic:
            check(L.mci_set_deterministic(self.p, 1))
        nd, no, ps, tm, lds = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
        check(L.mci_problem_info(self.p, C.byref(nd), C.byref(no), C.byref(ps), C.byref(tm), C.byref(lds)))
        self.ndraw, self.nobs, self.packed_size, self.table_mode, self.lds_bytes = nd.value, no.value, ps.value, tm.value, lds.value
        if device >= 0 and not np.allclose(config._reweight0, 1.0 / (config.N + 1)):
            r = np.ascontiguousarray(config._reweight0)
            check(L.mci_set_reweight(self.p, _dp(r), len(r)))
        for i, lf in enumerate(leaves):
            lf._engine, lf._leaf_index = self, i

    def _make_host_callback(self, fn, inplace=False):
        """ctypes trampoline: draw-major x[k*n + i] -> numpy views -> fn(x, config) -> w[q*n + i]; inplace: fn(x, weights, config)
        writes into a view of w itself (vegas/montecarlo.jl:140-141).  A closure written per sample with Python branches on its draws
        (`1.0 if x[0] ** 2 + x[1] ** 2 < 1 else 0.0`: the reference's own style) cannot take a batch -- numpy refuses the truth value
        of an array -- and is then called sample by sample (slow; such a closure normally never gets here: the tracer writes its
        branches out as selects)."""
        config = self.config
        nc = config.ncomp
        state = {"per_sample": False}

        def views(X, n):
            return self._pool_views(X, n)

        def batch(X, W, n):
            arg = views(X, n)
            if inplace:
                if nc == 2:
                    Z = np.zeros((config.N, n), dtype=complex)
                    fn(arg, Z, config)
                    W[0::2], W[1::2] = Z.real, Z.imag
                else:
                    W[:] = 0.0
                    fn(arg, W, config)
                return
            out = fn(arg, config)
            if config.N == 1 and not isinstance(out, (tuple, list)):
                out = (out,)
            assert len(out) == config.N, "the integrand must return one value per integrand"
            for i, o in enumerate(out):
                o = np.broadcast_to(np.asarray(o), (n,))
                if nc == 2:
                    W[2 * i] = o.real
                    W[2 * i + 1] = o.imag
                else:
                    W[i] = o

        def per_sample(X, W, n):
            Z = np.zeros((config.N, n), dtype=complex if nc == 2 else float)
            for j in range(n):
                arg = self._pool_views(X[:, j:j + 1], 1, scalar=True)
                if inplace:
                    w = np.zeros(config.N, dtype=Z.dtype)
                    fn(arg, w, config)
                    Z[:, j] = w
                else:
                    out = fn(arg, config)
                    if config.N == 1 and not isinstance(out, (tuple, list)):
                        out = (out,)
                    assert len(out) == config.N, "the integrand must return one value per integrand"
                    for i, o in enumerate(out):
                        Z[i, j] = o
            if nc == 2:
                W[0::2], W[1::2] = Z.real, Z.imag
            else:
                W[:] = Z

        def cb(xp, wp, n, ndraw, nw, user):
            try:
                X = np.ctypeslib.as_array(xp, shape=(ndraw, n))
                W = np.ctypeslib.as_array(wp, shape=(nw, n))
                if not state["per_sample"]:
                    try:
                        batch(X, W, n)
                        return 0
                    except (ValueError, TypeError, IndexError) as e:
                        # a closure written per sample like the reference's: a Python branch on a draw ("The truth value of an array
                        # with more than one element is ambiguous"), a list indexed with a Discrete draw ("only integer scalar arrays
                        # can be converted to a scalar index"), ...: sample by sample from here on (an error of its own comes again)
                        if n <= 1:
                            raise
                        _slow_path_warning("integrand", "sample", e)
                        state["per_sample"] = True
                per_sample(X, W, n)
                return 0
            except Exception:   # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        return cb

    def _make_host_indexed_callback(self, fn):
        """ctypes trampoline of the `integrand(idx, var, config)` form: one call of fn per integrand index some chain asks for,
        over the chains that ask for it"""
        config = self.config
        nc = config.ncomp
        state = {"per_sample": False}

        def cb(ip, xp, wp, n, ndraw, ncomp, user):
            try:
                idx = np.ctypeslib.as_array(ip, shape=(n,))
                X = np.ctypeslib.as_array(xp, shape=(ndraw, n))
                W = np.ctypeslib.as_array(wp, shape=(ncomp, n))
                for i in np.unique(idx[idx >= 0]):
                    sel = np.nonzero(idx == i)[0]
                    whole = len(sel) == n
                    Xs = X if whole else np.ascontiguousarray(X[:, sel])
                    o = None
                    if not state["per_sample"]:
                        try:
                            o = fn(int(i), self._pool_views(Xs, len(sel)), config)
                        except (ValueError, TypeError, IndexError) as e:   # a closure written per sample: sample by sample (see _make_host_callback)
                            if len(sel) <= 1:
                                raise
                            _slow_path_warning("integrand", "sample", e)
                            state["per_sample"] = True
                    if o is None:
                        o = np.array([fn(int(i), self._pool_views(np.ascontiguousarray(Xs[:, j:j + 1]), 1, scalar=True), config) for j in range(len(sel))])
                    o = np.broadcast_to(np.asarray(o), (len(sel),))
                    if nc == 2:
                        W[0, sel], W[1, sel] = o.real, o.imag
                    else:
                        W[0, sel] = o
                return 0
            except Exception:   # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        return cb

    def _pool_views(self, X, n, scalar=False):
        """draw-major [ndraw, n] -> what the reference hands a closure: the pool itself with one variable type, else a tuple of pools
        (scalar: one sample without the batch axis, for a closure that is called sample by sample).  A Discrete pool holds integers like
        the reference's (variable.jl:283: `grid[bin[0] - 1]`, `obs[0][ext[0] - 1] += w` index with them as they are); a CompositeVar
        is indexed [leaf][slot] (variable.jl:436-447: `x, y = cvar`) -- one array when its leaves are of one kind, else a tuple of
        per-leaf arrays; a pool with `offset` gets that many leading zero slots: the reference's closures address X[i + offset]
        (variable.jl:577, test/montecarlo.jl:19-32)."""
        layout = self.config.pool_layout()

        def typed(a, kind):
            return np.rint(a).astype(np.int64) if kind == "d" else a

        def pool(k0, md, nl, off, composite, kinds):
            a = X[k0:k0 + md * nl].reshape((md, n) if nl == 1 and not composite else (md, nl, n))
            if off:
                a = np.concatenate([np.zeros((off,) + a.shape[1:]), a])
            if composite:                  # [leaf][slot]
                a = a.transpose(1, 0, 2)
                if len(set(kinds)) > 1:
                    return tuple(typed(a[l][..., 0] if scalar else a[l], kinds[l]) for l in range(nl))
            return typed(a[..., 0] if scalar else a, kinds[0])
        if len(layout) == 1 and layout[0][2:] == (1, 0, False, "c"):
            return X[:, 0] if scalar else X
        arg = tuple(pool(*p) for p in layout)
        return arg[0] if len(arg) == 1 else arg

    def _make_host_measure_callback(self, fn):
        """ctypes trampoline: one block's draws and relative weights -> numpy views -> fn(x, obs, weights, config) -> obs[nobs].
        The closure is called once with the block's records as arrays (the batch form: `obs[0][0] += weights[0].sum()`); one written
        per record like the reference's (`obs[1][1] += weights[1]`, vegas/montecarlo.jl:156-161) raises on arrays and is then called
        record by record.  `obs[i][bins] += w` with an integer ARRAY of bins (a Discrete draw over the records) accumulates every
        record, repeated bins included (_HostObs)."""
        config = self.config
        nc = config.ncomp
        dt = complex if nc == 2 else float
        state = {"per_record": False}

        def cb(xp, rp, n, stride, ndraw, nw, block, op, nobs, user):
            try:
                X = np.ctypeslib.as_array(xp, shape=(ndraw, stride))[:, :n]
                R = np.ctypeslib.as_array(rp, shape=(nw, stride))[:, :n]
                O = np.ctypeslib.as_array(op, shape=(nobs,))
                weights = [R[2 * i] + 1j * R[2 * i + 1] for i in range(config.N)] if nc == 2 else [R[i] for i in range(config.N)]
                obs = None
                if not state["per_record"]:
                    obs = [_HostObs(shape, dt) for shape in config.obs_shape]
                    try:
                        fn(self._pool_views(X, n), obs, weights, config)
                    except (ValueError, TypeError, IndexError) as e:
                        if n <= 1:
                            raise
                        _slow_path_warning("measure", "record", e)
                        state["per_record"], obs = True, None
                if obs is None:
                    obs = [np.zeros(shape, dtype=dt) for shape in config.obs_shape]
                    for j in range(n):
                        fn(self._pool_views(X[:, j:j + 1], 1, scalar=True), obs, [w[j] for w in weights], config)
                _store_obs(O, obs, config.obs_nbin, nc)
                return 0
            except Exception:   # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        return cb

    def _make_host_measure_indexed_callback(self, fn):
        """ctypes trampoline of the `measure(idx, var, obs, relative_weight, config)` form: one call of fn per integrand index that
        some record of the block belongs to, over those records (record by record for a closure that raises on arrays, see above)"""
        config = self.config
        nc = config.ncomp
        dt = complex if nc == 2 else float
        state = {"per_record": False}

        def cb(ip, xp, rp, n, stride, ndraw, ncomp, block, op, nobs, user):
            try:
                idx = np.ctypeslib.as_array(ip, shape=(n,))
                X = np.ctypeslib.as_array(xp, shape=(ndraw, stride))[:, :n]
                R = np.ctypeslib.as_array(rp, shape=(ncomp, stride))[:, :n]
                O = np.ctypeslib.as_array(op, shape=(nobs,))
                obs, off = [], 0
                for shape, nb in zip(config.obs_shape, config.obs_nbin):   # the block's observables so far (the library calls once per integrand)
                    o = np.array(O[off:off + nb])
                    obs.append(((o[0::2] + 1j * o[1::2]) if nc == 2 else o.astype(dt)).reshape(shape).view(_HostObs))
                    off += nb
                w = (R[0] + 1j * R[1]) if nc == 2 else R[0]
                for i in np.unique(idx[idx >= 0]):
                    sel = np.nonzero(idx == i)[0]
                    whole = len(sel) == n
                    Xs = X if whole else np.ascontiguousarray(X[:, sel])
                    ws = w if whole else w[sel]
                    if not state["per_record"]:
                        before = [np.array(o) for o in obs]
                        try:
                            fn(int(i), self._pool_views(Xs, len(sel)), obs, ws, config)
                            continue
                        except (ValueError, TypeError, IndexError) as e:
                            if len(sel) <= 1:
                                raise
                            _slow_path_warning("measure", "record", e)
                            state["per_record"] = True
                            for o, q in zip(obs, before):
                                np.ndarray.__setitem__(o, slice(None), q)
                    plain = [o.view(np.ndarray) for o in obs]
                    for j in range(len(sel)):
                        fn(int(i), self._pool_views(np.ascontiguousarray(Xs[:, j:j + 1]), 1, scalar=True), plain, ws[j], config)
                _store_obs(O, obs, config.obs_nbin, nc)
                return 0
            except Exception:   # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        return cb

    def close(self):
        if getattr(self, "p", None):
            lib().mci_problem_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- kernels -------------------------------------------------------------------------------
    @staticmethod
    def _kernel_code(solver):
        return {"vegas_persistent": 3, "vegasmc_lanes": 5, "mcmc_lanes": 6, "vegas_strat": 7, "vegas_sweep": 8, "vegas_sweep_leaves": 9, "vegas_sweep_strat": 10,
                "vegasmc_sweep": 11, "mcmc_sweep": 12, "vegasmc_sweep_carry": 13, "mcmc_sweep_carry": 14, "vegas_big": 15,
                "vegas_sweep_strat_leaves": 16, "vegas_sweep_until": 17, "vegas_sweep_leaves_until": 18, "vegasmc_sweep_resume": 19, "mcmc_sweep_resume": 20,
                "vegas_persistent_until": 21}.get(solver) or _lib.SOLVERS[solver]

    def compile(self, solver="vegas"):
        """solver: "vegas" | "vegasmc" | "mcmc" | "vegas_persistent" (the persistent :vegas kernel, layouts with one Continuous leaf) |
        "vegasmc_lanes" | "mcmc_lanes" (the chain solvers' kernels with several lanes per chain, csrc/mci_spec.h) | "vegas_strat" (the
        stratified :vegas kernel, csrc/mci_strat.h; the problem must be stratified: set_stratification) | "vegas_sweep" (the kernel of
        integrate_sweep, csrc/mci_sweep.h; layouts sweep_supported accepts) | "vegas_sweep_leaves" (the sweep kernel of a problem with
        several variable leaves, csrc/mci_sweep_leaves.h; after set_sweep_leaves("all")) | "vegas_sweep_strat" (the kernel of
        integrate_sweep_strat, csrc/mci_sweep_strat.h; stratified problems sweep_strat_supported accepts) | "vegasmc_sweep" (the kernel of
        integrate_sweep_chains, csrc/mci_sweep_chains.h; layouts sweep_chains_supported accepts) | "mcmc_sweep" (the kernel of
        integrate_sweep_mcmc, the same header's :mcmc instantiation; layouts sweep_mcmc_supported accepts) | "vegasmc_sweep_carry" |
        "mcmc_sweep_carry" (the same two kernels with chains carried from iteration to iteration: set_sweep_chain_carry) | "vegas_big" (the
        :vegas kernel with sixteen histogram copies in 1024-thread workgroups that big launches of eight-copy layouts run) |
        "vegas_sweep_strat_leaves" (the kernel of integrate_sweep_strat for a stratified problem with several Continuous leaves,
        csrc/mci_sweep_strat_leaves.h; after set_sweep_strat_leaves("all")) | "vegas_sweep_until" | "vegas_sweep_leaves_until" (the kernels
        of integrate_sweep_until: "vegas_sweep" and "vegas_sweep_leaves" with a target error per point) | "vegasmc_sweep_resume" |
        "mcmc_sweep_resume" (the two carried kernels with a first iteration that continues the chains of the call before: state=) |
        "vegas_persistent_until" (the persistent :vegas kernel with a target error, csrc/mci_persist_until.h: what integrate(..., rtol= |
        atol=) launches where a fixed call launches "vegas_persistent")"""
        check(lib().mci_compile_solver(self.p, self._kernel_code(solver)))

    def code_object(self, solver="vegas"):
        """kernel-cache file holding the solver's gfx950 code object (after compile / the first run)"""
        buf = C.create_string_buffer(4096)
        check(lib().mci_kernel_code_object(self.p, self._kernel_code(solver), buf, len(buf)))
        return buf.value.decode()

    def set_kernel_timing(self, mode=-1):
        """HIP events around every sample launch (kernel_times_ms): -1 launches of >= 2^20 samples (default), 0 never, 1 always"""
        check(lib().mci_set_kernel_timing(self.p, int(mode)))

    def histogram_copies(self):
        """interleaved copies of the LDS histograms in the :vegas sample kernel (1 = the plain layout)"""
        n = C.c_int32()
        check(lib().mci_get_histogram_copies(self.p, C.byref(n)))
        return n.value

    def check_status(self):
        """synchronise and raise what the device flagged (normalization / histogram / chain start errors)"""
        check(lib().mci_check_status(self.p))

    def set_launch(self, threads=0, wg_per_block=-1):
        check(lib().mci_set_launch(self.p, threads, wg_per_block))

    def run(self, solver, nevalperblock, block_lo, block_hi, iteration, seed, measurefreq=1, nchain=0, thermal_ratio=0.1):
        check(lib().mci_iteration_run(self.p, _lib.SOLVERS[solver], int(nevalperblock), int(block_lo), int(block_hi),
                                      int(iteration), int(seed), int(measurefreq), int(nchain), float(thermal_ratio)))

    def reduce(self):
        check(lib().mci_iteration_reduce(self.p))

    def finish(self, solver, block_total, adapt=True, gamma=1.0, want_stats=True):
        if not want_stats:
            check(lib().mci_iteration_finish(self.p, _lib.SOLVERS[solver], int(block_total), 1 if adapt else 0, gamma, None, None))
            return None, None
        m, e = np.empty(self.nobs), np.empty(self.nobs)
        check(lib().mci_iteration_finish(self.p, _lib.SOLVERS[solver], int(block_total), 1 if adapt else 0, gamma, _dp(m), _dp(e)))
        return m, e

    def iteration(self, solver, nevalperblock, block_lo, block_hi, iteration, seed, measurefreq=1, nchain=0, thermal_ratio=0.1):
        """run + read back the local packed buffer [obsSum|obsSqSum|normalization|neval|visited|histograms]"""
        self.run(solver, nevalperblock, block_lo, block_hi, iteration, seed, measurefreq, nchain, thermal_ratio)
        return self.get_packed()

    def iteration_log(self, nrows):
        """statistics head of the last nrows finished iterations, [nrows, 2*nobs+2+N+1] (oldest first)"""
        nstat = 2 * self.nobs + 2 + self.config.N + 1
        out = np.empty((nrows, nstat))
        check(lib().mci_get_iteration_log(self.p, int(nrows), _dp(out)))
        return out

    def reserve_iterations(self, rows):
        """room for `rows` more iterations in the device-side log, so that none of them synchronises to grow it"""
        check(lib().mci_reserve_iteration_log(self.p, int(rows)))

    def get_packed(self, reduce_size=False):
        """the packed buffer [statistics | histograms | propose | accept]; reduce_size: with the 64 :mcmc holding-time counts behind it --
        what an external reducer sums over the ranks (mci_reduce_size)"""
        out = np.empty(self.reduce_size if reduce_size else self.packed_size)
        check(lib().mci_get_packed(self.p, _dp(out), len(out)))
        return out

    @property
    def reduce_size(self):
        return self.packed_size + 64

    def external_reduce_done(self):
        """an external reducer has summed reduce_size doubles of the packed buffer over the ranks; see mci_external_reduce_done"""
        check(lib().mci_external_reduce_done(self.p))

    def comm_collectives(self):
        """(ncclAllReduce calls the library has issued on this engine's context, element count of the last one)"""
        n, c = C.c_int64(), C.c_int64()
        check(lib().mci_comm_collectives(context(self.device), C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def set_packed(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        check(lib().mci_set_packed(self.p, _dp(a), len(a)))

    def packed_device_ptr(self):
        return lib().mci_packed_device_ptr(self.p)

    def hold_histogram(self):
        """:mcmc: chains of the last launch by bit_width(longest holding time) -- what the automatic chain length follows"""
        out = (C.c_uint64 * 64)()
        check(lib().mci_get_hold_histogram(self.p, out))
        return np.array(list(out), dtype=np.uint64)

    def resample(self, curr_old, rw_now, rw_used, n_new, w_chain=None):
        """test hook (csrc/mci_debug.h mci_debug_resample): the carried chains' resampler kernel on its own over curr_old [nblocks, n_old]
        (w_chain [nblocks, n_old]: a weight per stored chain instead of rw_now / rw_used [nd]) -> (src [nblocks, n_new], W [nblocks,
        n_old]); this engine gives its device only, its own stored chains stay as they are"""
        co = np.ascontiguousarray(curr_old, dtype=np.int32)
        a, b = np.ascontiguousarray(rw_now, dtype=np.float64), np.ascontiguousarray(rw_used, dtype=np.float64)
        wc = None if w_chain is None else np.ascontiguousarray(w_chain, dtype=np.float64)
        if co.ndim != 2 or a.shape != b.shape or a.ndim != 1 or (wc is not None and wc.shape != co.shape):
            raise ValueError("curr_old [nblocks, n_old], rw_now and rw_used [nd], w_chain None or shaped like curr_old")
        nblocks, n_old = co.shape
        src = np.full((nblocks, max(int(n_new), 0)), -1, dtype=np.int32)
        W = np.full((nblocks, n_old), np.nan)
        check(lib().mci_debug_resample(self.p, nblocks, n_old, int(n_new), len(a), co.ctypes.data_as(c_int32_p), _dp(a), _dp(b),
                                       None if wc is None else _dp(wc), src.ctypes.data_as(c_int32_p), _dp(W)))
        return src, W

    def merge_shape(self):
        """the problem's shape as the merge kernels see it (csrc/mci_debug.h mci_debug_merge_shape; no device needed): a dict of nobs, ni,
        ncols, nbin, npa, nstat, maxn (bins of the largest leaf) and leaves [(offset into the histogram section, bins)]"""
        sh = np.zeros(8, dtype=np.int32)
        check(lib().mci_debug_merge_shape(self.p, sh.ctypes.data_as(c_int32_p), None))
        lv = np.zeros((int(sh[6]), 2), dtype=np.int32)
        check(lib().mci_debug_merge_shape(self.p, sh.ctypes.data_as(c_int32_p), lv.ctypes.data_as(c_int32_p)))
        out = dict(zip(("nobs", "ni", "ncols", "nbin", "npa", "nstat"), (int(v) for v in sh[:6])))
        out["maxn"], out["leaves"] = int(sh[7]), [(int(a), int(b)) for a, b in lv]
        return out

    def merge_rows(self, nblocks, wg_per_block, part_cols, part_hist=None, ghist=None, part_pa=None, hold=None, obs=None, hist_no_offset=False,
                   block_means=True, path="finalize", train=None, grids=None, tables=None):
        """test hook (csrc/mci_debug.h mci_debug_merge): the merge kernels on their own over rows the caller made up -- part_cols [nrows,
        ncols], part_hist [hist_rows, nbin] (through k_hist_stage1) or ghist [k, nbin] (use_ghist = k), part_pa [nrows, 2 npa], hold [64]
        (uint64), obs [nblocks, nobs] (k_add_host_obs runs first); path "finalize" (k_finalize) | "finish" (k_finish, told to merge only).
        -> dict of packed [reduce_size], stage1 [32, nbin], scratch [nblocks, ncols], block_means [nblocks, nobs] (None if not wanted),
        status, part_cols [nrows, ncols] and ghist [k + 1, nbin] (the last row: the hook's NaN guard) as left behind.  This engine gives its
        device and its shape only; nothing of its own state is read or written.
        train (path "finish" only): a walk as set_train_walk names them ("scan", "serial", "serial_general", "serial_wrong_decision") --
        k_finish then refines every adapting leaf from the histogram it merged, on tables of the hook's own: grids = the old grid of every
        Continuous leaf in leaf order, tables = (distribution, accumulation) of every Discrete leaf in leaf order.  The dict gains grids and
        tables as k_finish left them (same order) and walk_counts (slots, general form)"""
        sh = self.merge_shape()
        pc = np.ascontiguousarray(part_cols, dtype=np.float64)
        ph = None if part_hist is None else np.ascontiguousarray(part_hist, dtype=np.float64)
        gh = None if ghist is None else np.ascontiguousarray(ghist, dtype=np.float64)
        pa = None if part_pa is None else np.ascontiguousarray(part_pa, dtype=np.float64)
        hd = None if hold is None else np.ascontiguousarray(hold, dtype=np.uint64)
        ob = None if obs is None else np.ascontiguousarray(obs, dtype=np.float64)
        nblocks, wg_per_block = int(nblocks), int(wg_per_block)
        if (pc.ndim != 2 or pc.shape[1] != sh["ncols"] or (ph is not None and (ph.ndim != 2 or ph.shape[1] != sh["nbin"]))
                or (gh is not None and (gh.ndim != 2 or gh.shape[1] != sh["nbin"])) or (pa is not None and pa.shape != (pc.shape[0], 2 * sh["npa"]))
                or (hd is not None and hd.shape != (64,)) or (ob is not None and ob.shape != (nblocks, sh["nobs"])) or path not in ("finalize", "finish")):
            raise ValueError("part_cols [nrows, ncols], part_hist [hist_rows, nbin], ghist [k, nbin], part_pa [nrows, 2 npa], hold [64], "
                             "obs [nblocks, nobs], path 'finalize' or 'finish'")
        nrows, k = pc.shape[0], 0 if gh is None else gh.shape[0]
        nb = max(min(nblocks, nrows), 0)   # (more blocks than rows: refused before anything is written)
        out = dict(packed=np.full(self.reduce_size, np.nan), stage1=np.full((32, sh["nbin"]), np.nan), scratch=np.full((nb, sh["ncols"]), np.nan),
                   block_means=np.full((nb, sh["nobs"]), np.nan) if block_means else None, part_cols=np.full(pc.shape, np.nan),
                   ghist=np.full((k + 1, sh["nbin"]), np.nan))
        status = C.c_int32(-1)
        io = _lib.DebugMergeIO(nblocks, wg_per_block, nrows, 0 if ph is None else ph.shape[0], k, 1 if hist_no_offset else 0,
                               0 if path == "finalize" else 1, _dp(pc), None if ph is None else _dp(ph), None if gh is None else _dp(gh),
                               None if pa is None else _dp(pa), None if hd is None else hd.ctypes.data_as(C.POINTER(C.c_uint64)),
                               None if ob is None else _dp(ob), _dp(out["packed"]), _dp(out["stage1"]), _dp(out["scratch"]),
                               None if out["block_means"] is None else _dp(out["block_means"]), C.pointer(status), _dp(out["part_cols"]),
                               _dp(out["ghist"]))
        if train is not None:
            if path != "finish" or train not in ("scan", "serial", "serial_general", "serial_wrong_decision"):
                raise ValueError("train: path 'finish' and a walk of set_train_walk")
            cont = [lf for lf in self.config.leaves if isinstance(lf, ContinuousVar)]
            disc = [lf for lf in self.config.leaves if not isinstance(lf, (ContinuousVar, FermiK))]
            gs = [np.ascontiguousarray(g, dtype=np.float64) for g in (grids or [])]
            ts = [(np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)) for d, a in (tables or [])]
            if ([g.shape for g in gs] != [(lf.ninc,) for lf in cont]
                    or [(d.shape, a.shape) for d, a in ts] != [((lf.upper - lf.lower + 1,), (lf.upper - lf.lower + 2,)) for lf in disc]):
                raise ValueError("grids: one old grid per Continuous leaf; tables: (distribution [K], accumulation [K + 1]) per Discrete leaf")
            cat = lambda xs: np.concatenate(xs) if xs else np.zeros(1)
            gin, din, ain = cat(gs), cat([d for d, a in ts]), cat([a for d, a in ts])
            gout, dout, aout = np.full(gin.shape, np.nan), np.full(din.shape, np.nan), np.full(ain.shape, np.nan)
            counts = (C.c_int64 * 2)(-1, -1)
            io.do_train, io.train_walk = 1, {"scan": 0, "serial": 1, "serial_general": 2, "serial_wrong_decision": 3}[train]
            io.grids, io.dists, io.accs, io.grids_out, io.dists_out, io.accs_out = _dp(gin), _dp(din), _dp(ain), _dp(gout), _dp(dout), _dp(aout)
            io.walk_counts = C.cast(counts, C.POINTER(C.c_int64))
        check(lib().mci_debug_merge(self.p, C.byref(io)))
        out["status"] = int(status.value)
        if train is not None:
            gsplit = np.split(gout, np.cumsum([g.size for g in gs])[:-1]) if gs else []
            dsplit = np.split(dout, np.cumsum([d.size for d, a in ts])[:-1]) if ts else []
            asplit = np.split(aout, np.cumsum([a.size for d, a in ts])[:-1]) if ts else []
            out["grids"], out["tables"], out["walk_counts"] = gsplit, list(zip(dsplit, asplit)), (int(counts[0]), int(counts[1]))
        return out

    def strat_alloc_rows(self, d, nsamp, uniform=False):
        """test hook (csrc/mci_debug.h mci_debug_strat_alloc): k_strat_alloc's three launches on their own over d [ncube] made up by the
        caller -> (off [ncube + 1] int64, tsum [2 ntile + 2] = tile sums | tile bases | total | uniform flag).  This engine gives its
        device only and need not be stratified; its own plan and allocation stay as they are"""
        d = np.ascontiguousarray(d, dtype=np.float64)
        if d.ndim != 1:
            raise ValueError("d [ncube]")
        ntile = max(min(-(-d.size // 256), 1024), 0)
        off = np.full(d.size + 1, -1, dtype=np.int64)
        tsum = np.full(2 * ntile + 2, np.nan)
        check(lib().mci_debug_strat_alloc(self.p, _dp(d), d.size, int(nsamp), 1 if uniform else 0, off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(tsum)))
        return off, tsum

    def strat_reduce_rows(self, off, part, rec_h, rec_s, dnext, beta, log_row=True):
        """test hook (csrc/mci_debug.h mci_debug_strat_reduce): k_strat_reduce on its own over off [ncube + 1], part [nchunk, 2 nw], rec_h
        [nchunk, 2], rec_s [nchunk, 2, 2 nw] and dnext [ncube] (the fill the cut hypercubes' d_h are written into) -> dict of out [2 nw],
        log_row [2 nw] (None if not asked for: the kernel is then given no log row) and dnext [ncube] as the kernel left it"""
        off = np.ascontiguousarray(off, dtype=np.int64)
        part = np.ascontiguousarray(part, dtype=np.float64)
        rec_h = np.ascontiguousarray(rec_h, dtype=np.int64)
        rec_s = np.ascontiguousarray(rec_s, dtype=np.float64)
        dn = np.array(dnext, dtype=np.float64, order="C")
        if (off.ndim != 1 or part.ndim != 2 or part.shape[1] % 2 or rec_h.shape != (part.shape[0], 2) or rec_s.shape != (part.shape[0], 2, part.shape[1])
                or dn.shape != (off.size - 1,)):
            raise ValueError("off [ncube + 1], part [nchunk, 2 nw], rec_h [nchunk, 2], rec_s [nchunk, 2, 2 nw], dnext [ncube]")
        nchunk, nw = part.shape[0], part.shape[1] // 2
        out = np.full(2 * nw, np.nan)
        row = np.full(2 * nw, np.nan) if log_row else None
        i64 = C.POINTER(C.c_int64)
        io = _lib.DebugStratReduceIO(off.size - 1, nchunk, nw, float(beta), off.ctypes.data_as(i64), _dp(part), rec_h.ctypes.data_as(i64), _dp(rec_s),
                                     _dp(dn), _dp(out), None if row is None else _dp(row))
        check(lib().mci_debug_strat_reduce(self.p, C.byref(io)))
        return dict(out=out, log_row=row, dnext=dn)

    def strat_remap_rows(self, n_old, n_new, e, d_old):
        """test hook (csrc/mci_debug.h mci_debug_strat_remap): k_strat_remap on its own: d_old [prod n_old] on the plan n_old -> d_new
        [prod n_new] on the plan n_new, raised to e (e == 1 copies the bits)"""
        no, nn = np.ascontiguousarray(n_old, dtype=np.int32), np.ascontiguousarray(n_new, dtype=np.int32)
        d = np.ascontiguousarray(d_old, dtype=np.float64)
        if no.ndim != 1 or no.shape != nn.shape or d.ndim != 1:
            raise ValueError("n_old and n_new [ndim], d_old [prod n_old]")
        # (a plan the hook refuses is refused before anything is read or written)
        ok = 1 <= no.size <= 32 and min(no.min(), nn.min()) >= 1 and max(np.prod(no, dtype=np.float64), np.prod(nn, dtype=np.float64)) < 2 ** 31
        if ok and d.size != int(np.prod(no, dtype=np.int64)):
            raise ValueError("n_old and n_new [ndim], d_old [prod n_old]")
        out = np.full(int(np.prod(nn, dtype=np.int64)) if ok else 1, np.nan)
        check(lib().mci_debug_strat_remap(self.p, no.size, no.ctypes.data_as(c_int32_p), nn.ctypes.data_as(c_int32_p), float(e), _dp(d), _dp(out)))
        return out

    def sweep_resample_lds(self):
        """stored chains per block up to which a carried sweep point's resampler keeps its running weights in LDS (csrc/mci_debug.h
        mci_debug_sweep_resample_lds)"""
        n = C.c_int64()
        check(lib().mci_debug_sweep_resample_lds(self.p, C.byref(n)))
        return int(n.value)

    def stream(self):
        """the library's hipStream_t (as an integer), for callers that order their own work with ours"""
        return lib().mci_ctx_stream(context(self.device)) or 0

    def save_state(self, path):
        """grids, distributions and reweight -> MCISTATE file (resume across processes); an engine that carries its stratified
        allocation (set_stratification(carry=True)) adds it: one double per hypercube, up to 128 MB at the default cap"""
        check(lib().mci_save_state(self.p, str(path).encode()))

    def load_state(self, path):
        check(lib().mci_load_state(self.p, str(path).encode()))

    def train(self):
        check(lib().mci_train(self.p))

    def set_rng_rounds(self, rounds):
        """Philox4x32 rounds of every stream: 10 (default) or 7 (opt-in, 30 % less generator work); see mci_set_rng_rounds"""
        check(lib().mci_set_rng_rounds(self.p, int(rounds)))

    def set_rng_bits(self, bits):
        """:vegas sample stream: 52 (default, the resolution of rand(Float64)) or 32 random bits per draw; see mci_set_rng_bits"""
        check(lib().mci_set_rng_bits(self.p, int(bits)))

    def set_deterministic(self, on=True):
        """bit-identical results for a fixed seed, run to run (one LDS histogram copy per wave, fixed merge orders); see
        mci_set_deterministic"""
        check(lib().mci_set_deterministic(self.p, 1 if on else 0))

    def set_chain_carry(self, mode):
        """chain solvers with many chains per block: "auto" (default) / "on" -- the next iteration of the same solver over the same
        blocks continues the chains of the previous one (:mcmc: resampled to the reweight factors doReweight! has just moved) -- or
        "off" (every launch draws new starts and burns them in); see mci_set_chain_carry"""
        check(lib().mci_set_chain_carry(self.p, {"auto": -1, "off": 0, "on": 1, -1: -1, 0: 0, 1: 1}[mode]))

    def set_iteration_counted(self, counted):
        """for a loop over run / reduce / finish (integrate() with several ranks): the launches that follow enter the final average
        (iteration >= ignore); see mci_set_iteration_counted"""
        check(lib().mci_set_iteration_counted(self.p, 1 if counted else 0))

    def set_persistent(self, mode):
        """launch-bound :vegas calls of integrate() as ONE persistent launch: "auto" (default), "off" or "on" (whenever the layout
        allows, whatever the size); see mci_set_persistent"""
        check(lib().mci_set_persistent(self.p, {"auto": -1, "off": 0, "on": 1, -1: -1, 0: 0, 1: 1}[mode]))

    def last_integrate_persistent(self):
        """did the last integrate() of this engine run as one persistent launch?"""
        v = C.c_int32()
        check(lib().mci_last_integrate_persistent(self.p, C.byref(v)))
        return bool(v.value)

    def last_chain_launch(self):
        """(chains per block, continued the previous launch?) of the last chain-solver launch"""
        n, c = C.c_int64(), C.c_int32()
        check(lib().mci_last_chain_launch(self.p, C.byref(n), C.byref(c)))
        return int(n.value), bool(c.value)

    def set_chain_speculation(self, lanes=-1, accept=0.0, max_accepts=-1):
        """several lanes per chain (csrc/mci_spec.h): lanes -1 automatic, 1 never, 2..64 forced; the acceptance the speculation tree
        is built for and the most accept edges on a way through it (<= 0 / < 0: the solver's defaults); see mci_set_chain_speculation"""
        check(lib().mci_set_chain_speculation(self.p, int(lanes), float(accept), int(max_accepts)))

    def last_chain_speculation(self):
        """(lanes per chain, accept levels of the tree) of the last chain-solver launch; (1, 0) = one lane per chain"""
        g, m = C.c_int32(), C.c_int32()
        check(lib().mci_last_chain_speculation(self.p, C.byref(g), C.byref(m)))
        return int(g.value), int(m.value)

    def chain_speculation_status(self, solver):
        """the self-check of the solver's several-lanes-per-chain code object: 0 not launched yet, 1 verified against the lane-per-chain
        kernel (now or by an earlier process: the marker in the kernel cache), -1 failed (this problem keeps one lane per chain), -2 did
        not compile; see mci_chain_speculation_status"""
        st = C.c_int32()
        check(lib().mci_chain_speculation_status(self.p, _lib.SOLVERS[solver], C.byref(st)))
        return int(st.value)

    def vegas_check_status(self):
        """(status, flags) of the self-check of this problem's :vegas code objects against the library's static :vegas kernel: status 0
        not looked at (nothing launched yet, or a path the check does not cover), 1 verified, -1 fell back to the conservative layout,
        -2 no layout agreed; flags bit 0 = observables not compared (a user measure), bit 1 = verified from a marker in the kernel
        cache, not in this process, bit 2 = the check's histogram was empty on both sides (not compared: status stays 0); see
        mci_vegas_check_status"""
        st, fl = C.c_int32(), C.c_int32()
        check(lib().mci_vegas_check_status(self.p, C.byref(st), C.byref(fl)))
        return int(st.value), int(fl.value)

    def vegas_check_launches(self):
        """launches made for the :vegas self-check of this problem so far; see csrc/mci_debug.h mci_debug_vegas_check_launches"""
        n = C.c_int64()
        check(lib().mci_debug_vegas_check_launches(self.p, C.byref(n)))
        return int(n.value)

    def vegas_check_reference(self, nevalperblock, block_lo, nblocks, iteration=0, seed=1234, measurefreq=1, x=None, jac=None, w=None):
        """(packed, (x mismatches, jac mismatches)): one iteration through the library's static :vegas kernel on its own, fed the samples
        x[n][ndraw], jac[n], w[n][ni * ncomp] (None: this problem's own sample dump); see csrc/mci_debug.h mci_debug_vegas_check"""
        packed = np.zeros(self.packed_size)
        bad = (C.c_int64 * 2)()
        ptr = [None, None, None]
        if x is not None:
            keep = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, jac, w)]
            ptr = [v.ctypes.data_as(_lib.c_double_p) for v in keep]
        check(lib().mci_debug_vegas_check(self.p, int(iteration), int(seed), int(nevalperblock), int(block_lo), int(nblocks), int(measurefreq),
                                          ptr[0], ptr[1], ptr[2], packed.ctypes.data_as(_lib.c_double_p), bad))
        return packed, (int(bad[0]), int(bad[1]))

    def vegas_check_layout(self):
        """the run-time layout table the static :vegas kernel is given for this problem (no device needed); see csrc/mci_debug.h
        mci_debug_vegas_check_layout"""
        head = (C.c_int32 * 8)()
        check(lib().mci_debug_vegas_check_layout(self.p, head, None, None, None, None))
        nd, ni = int(head[0]), int(head[1])
        draws, scales = (C.c_int32 * (6 * max(nd, 1)))(), (C.c_double * max(nd, 1))()
        own, obs = (C.c_uint64 * max(ni, 1))(), (C.c_int32 * (3 * max(ni, 1)))()
        check(lib().mci_debug_vegas_check_layout(self.p, head, draws, scales, own, obs))
        keys = ("kind", "off", "doff", "nbin", "boff", "hist")
        return dict(ndraw=nd, ni=ni, ncomp=int(head[2]), nobs=int(head[3]), ncols=int(head[4]), nbin=int(head[5]), covered=bool(head[6]),
                    with_obs=bool(head[7]),
                    draws=[dict(zip(keys, [int(draws[6 * k + j]) for j in range(6)]), scale=float(scales[k])) for k in range(nd)],
                    integrands=[dict(own=int(own[i]), obs_off=int(obs[3 * i]), obs_nbin=int(obs[3 * i + 1]), obs_bin_draw=int(obs[3 * i + 2]))
                                for i in range(ni)])

    def compile_chain_speculation(self, solver):
        """the several-lanes-per-chain kernel of "vegasmc" | "mcmc" (its own code object)"""
        check(lib().mci_compile_chain_speculation(self.p, _lib.SOLVERS[solver]))

    def set_train_walk(self, mode):
        """train!'s refinement walk: "serial" (the reference's recurrence), "scan" (prefix scan + bisection), "auto", or "serial_general"
        (the recurrence without the predicted decisions: what "serial" falls back to); see mci_set_train_walk.  "serial_wrong_decision" is
        the test hook of csrc/mci_debug.h: "serial" with one decision planted wrong, so that its check and the fall-back run"""
        check(lib().mci_debug_plant_wrong_decision(self.p, 1 if mode in ("serial_wrong_decision", 3) else 0))
        check(lib().mci_set_train_walk(self.p, {"auto": -1, "scan": 0, "serial": 1, "serial_general": 2, "serial_wrong_decision": 1, -1: -1, 0: 0, 1: 1, 2: 2, 3: 1}[mode]))

    def walk_counts(self):
        """(serial walks of train! run as slots with given decisions, walks in the general form) so far; see mci_debug_walk_counts"""
        out = (C.c_int64 * 2)()
        check(lib().mci_debug_walk_counts(self.p, out))
        return int(out[0]), int(out[1])

    def last_launch_cursor(self):
        """(did the last sample launch hand its ranges out by cursor?, the value its blocks' cursor words hold once every queued launch is
        through); see csrc/mci_debug.h mci_debug_vegas_cursor"""
        used, base = C.c_int32(0), C.c_uint64(0)
        check(lib().mci_debug_vegas_cursor(self.p, C.byref(used), C.byref(base)))
        return bool(used.value), int(base.value)

    def split_chunks(self):
        """(chunks, bytes of parked stream held at a time) of the last many-grid :vegas launch; see csrc/mci_debug.h mci_debug_split_chunks"""
        n, b = C.c_int64(), C.c_int64()
        check(lib().mci_debug_split_chunks(self.p, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def integrate(self, solver, neval, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0, measurefreq=1, seed=1234,
                  nchain=0, first_iteration=0, thermal_ratio=0.1, reweight_goal=None, target=None):
        """the whole loop inside the library (mci_integrate).  target = (rtol, atol, min_niter) (None entries: 0): the call stops at the
        first iteration n >= max(ignore + 2, min_niter) after which every statistics column has E <= max(atol, rtol |M|) -- M, E what
        the call would report with niter = n (mci_integrate_until); the dict then also carries `niter_run` (that n, or niter) and
        `converged`, its iter_mean / iter_std hold niter_run rows, and everything else is that of the call with niter = niter_run.
        Raises MCIError with the reason of integrate_until_supported()."""
        goal = None
        if reweight_goal is not None:
            self._goal = np.ascontiguousarray(reweight_goal, dtype=np.float64)
            goal = _dp(self._goal)
        a = _lib.IntegrateArgs(_lib.SOLVERS[solver], int(neval), int(niter), int(block), int(ignore), 1 if adapt else 0,
                               float(gamma), int(measurefreq), int(seed), int(nchain), int(first_iteration),
                               float(thermal_ratio), goal)
        n = self.nobs
        im, ie = np.zeros((niter, n)), np.zeros((niter, n))
        m, s, c2 = np.zeros(n), np.zeros(n), np.zeros(n)
        vis = np.zeros(self.config.N + 1)
        r = _lib.ResultC(niter, n, _dp(im), _dp(ie), _dp(m), _dp(s), _dp(c2), 0, 0.0, _dp(vis), 0, 0)
        nrun = None
        if target is None:
            check(lib().mci_integrate(self.p, C.byref(a), C.byref(r)))
        else:
            t, nrun = self._sweep_target(*target), C.c_int32(0)
            check(lib().mci_integrate_until(self.p, C.byref(a), C.byref(t), C.byref(r), C.byref(nrun)))
        dn, dl = C.c_int64(), C.c_int32()
        check(lib().mci_last_integrate_discarded(self.p, C.byref(dn), C.byref(dl)))
        out = dict(mean=m, stdev=s, chi2=c2, iter_mean=im, iter_std=ie, neval=r.neval, seconds=r.seconds, visited=vis,
                   correlated=bool(r.correlated), block_mean=None, warmup=int(r.warmup), neval_discarded=int(dn.value))
        if nrun is not None:
            niter = int(nrun.value)
            out["niter_run"] = niter
            out["iter_mean"], out["iter_std"] = im[:niter], ie[:niter]
            out["converged"] = self._integrate_until_met(out, ignore if ignore >= 0 else (1 if adapt else 0), t, len(im))
        if _lib.SOLVERS[solver] != _lib.VEGAS and out["correlated"]:
            # (only a run of carried chains needs them -- the block-lineage error of Result.with_ignore; a launch-bound default-size call is
            # spared the flush, the copy and the second synchronisation)
            out["block_mean"] = self.block_means(niter)[0]
        return out

    @staticmethod
    def _integrate_until_met(out, ignore, t, niter):
        """whether a call with a target met it: one that stopped below niter did by definition (the library's verdict, never
        second-guessed here); one that ran all niter iterations may have met it in the last -- the rule on what the call reports"""
        n = out["niter_run"]
        if n < niter:
            return True
        M, E = np.asarray(out["mean"]), np.asarray(out["stdev"])
        ok = np.isfinite(M) & np.isfinite(E) & (E <= np.maximum(t.atol, t.rtol * np.abs(M)))
        return bool(ok.all() and n >= max(ignore + 2, t.min_niter))

    def integrate_until_supported(self, solver="vegas", neval=10000, niter=10, block=16, measurefreq=1, rtol=0.0, atol=0.0, min_niter=0, **kw):
        """None when integrate(..., target=) takes this problem with these arguments and this target, else the reason
        (mci_integrate_until_supported: a negative or non-finite rtol / atol, min_niter < 0, several ranks, whatever mci_integrate refuses)"""
        t = _lib.SweepTarget(float(rtol), float(atol), int(min_niter))
        return self._sweep_refusal(lambda p, a, why, n: lib().mci_integrate_until_supported(p, a, C.byref(t), why, n), solver, neval, niter, block, measurefreq)

    def _integrate_args(self, solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration, nchain=0, thermal_ratio=0.1):
        return _lib.IntegrateArgs(_lib.SOLVERS[solver], int(neval), int(niter), int(block), int(ignore), 1 if adapt else 0, float(gamma),
                                  int(measurefreq), int(seed), int(nchain), int(first_iteration), float(thermal_ratio), None)

    def _sweep_refusal(self, query, solver, neval, niter, block, measurefreq, nchain=0, first_iteration=0, thermal_ratio=0.1):
        """None when the query (mci_sweep_supported | mci_sweep_strat_supported | mci_sweep_chains_supported | mci_sweep_mcmc_supported) takes
        this problem with these arguments, else its reason"""
        a = self._integrate_args(solver, neval, niter, block, -1, True, 1.0, measurefreq, 0, first_iteration, nchain, thermal_ratio)
        why = C.create_string_buffer(512)
        if query(self.p, C.byref(a), why, len(why)) == _lib.MCI_OK:
            return None
        return why.value.decode() or lib().mci_last_error().decode(errors="replace")

    def sweep_supported(self, solver="vegas", neval=10000, niter=10, block=16, measurefreq=1, **kw):
        """None when integrate_sweep takes this problem with these arguments, else the reason (mci_sweep_supported)"""
        return self._sweep_refusal(lib().mci_sweep_supported, solver, neval, niter, block, measurefreq)

    SWEEP_MAX_POINTS = 65536   # include/mci.h mci_integrate_sweep

    def set_sweep_leaves(self, mode="one"):
        """which problems integrate_sweep takes (mci_set_sweep_leaves): "one" (default) = one Continuous leaf; "all" = also any mix of
        Continuous and Discrete leaves whose tables, histograms and map fit a workgroup's LDS -- those run a kernel of their own
        (compile("vegas_sweep_leaves")); sweep_supported() names what still keeps a problem out"""
        if mode not in ("one", "all"):
            raise ValueError('set_sweep_leaves: "one" or "all", got %r' % (mode,))
        check(lib().mci_set_sweep_leaves(self.p, 1 if mode == "all" else 0))

    def set_sweep_strat_leaves(self, mode="one"):
        """which stratified problems integrate_sweep_strat takes (mci_set_sweep_strat_leaves): "one" (default) = one Continuous leaf;
        "all" = also several Continuous leaves (pools with ranges of their own, a composite with one grid per axis) whose tables, chunk
        and map fit a workgroup's LDS -- those run a kernel of their own (compile("vegas_sweep_strat_leaves")).  An opt-in of its own:
        set_sweep_leaves does not reach the stratified query.  sweep_strat_supported() names what still keeps a problem out"""
        if mode not in ("one", "all"):
            raise ValueError('set_sweep_strat_leaves: "one" or "all", got %r' % (mode,))
        check(lib().mci_set_sweep_strat_leaves(self.p, 1 if mode == "all" else 0))

    def set_sweep_chain_carry(self, on=True):
        """carried chains in integrate_sweep_chains / integrate_sweep_mcmc (mci_set_sweep_chain_carry; default off): every iteration of
        a point after its first continues the chains of the one before, resampled to the target train! and doReweight! have moved --
        what set_chain_carry(1) does for integrate(); :vegasmc with adapt=True from the third iteration on.  The first iteration of
        every call starts afresh: chain state does not travel between calls."""
        check(lib().mci_set_sweep_chain_carry(self.p, 1 if on else 0))

    def sweep_chain_carry(self):
        """what set_sweep_chain_carry set (mci_get_sweep_chain_carry)"""
        on = C.c_int32()
        check(lib().mci_get_sweep_chain_carry(self.p, C.byref(on)))
        return bool(on.value)

    def sweep_map_doubles(self):
        """doubles of one `maps` row of integrate_sweep (mci_sweep_map_doubles): the leaves in order, a Continuous leaf its grid, a
        Discrete leaf its accumulation and then its distribution"""
        n = C.c_int32()
        check(lib().mci_sweep_map_doubles(self.p, C.byref(n)))
        return int(n.value)

    def _split_sweep_map(self, row):
        """a flat `maps` row -> per leaf: the grid of a Continuous leaf, the distribution of a Discrete one"""
        out, o = [], 0
        for lf in self.config.leaves:
            if hasattr(lf, "ninc"):
                out.append(row[o:o + lf.ninc])
                o += lf.ninc
            else:   # accumulation [n + 1] | distribution [n]
                n = lf.upper - lf.lower + 1
                out.append(row[o + n + 1:o + 2 * n + 1])
                o += 2 * n + 1
        return out

    def integrate_sweep(self, solver="vegas", userdata=None, neval=10000, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0, measurefreq=1,
                        seed=1234, seeds=None, maps=None, first_iteration=0):
        """A parameter sweep in one launch (mci_integrate_sweep): userdata [P][nuserdata], one row per point -- what an ordinary call
        would have been given as the integrand's userdata.  Returns a list of P result dicts with the keys of integrate() plus `maps`
        (the point's map after its last iteration: the flat row of sweep_map_doubles() doubles), `maps_by_leaf` (that row leaf by leaf:
        the grid of a Continuous leaf, the distribution of a Discrete one) and `status` (the bits the device flagged for that point; 0 = none).  seed: the same
        for every point (common random numbers), or seeds = P of them; maps: None (every point starts from the engine's current map)
        or [P][grid points] starting maps (the layout of grid()).  The engine's own map, packed buffer and logs are not touched.  Raises MCIError naming the
        reason when the problem or the arguments cannot run as a sweep (sweep_supported): nothing else runs in its place."""
        ud, sd, mi, _ = self._sweep_inputs("integrate_sweep", userdata, seeds, maps)
        a = self._integrate_args(solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration)
        return self._sweep_call(lib().mci_integrate_sweep, a, ud.shape[0], niter, (ud, sd, mi), lambda P: ((), {}))

    @staticmethod
    def _sweep_target(rtol, atol, min_niter):
        return _lib.SweepTarget(float(0.0 if rtol is None else rtol), float(0.0 if atol is None else atol), int(0 if min_niter is None else min_niter))

    def sweep_until_supported(self, solver="vegas", neval=10000, niter=10, block=16, measurefreq=1, rtol=0.0, atol=0.0, min_niter=0, **kw):
        """None when integrate_sweep_until takes this problem with these arguments and this target, else the reason
        (mci_sweep_until_supported: whatever sweep_supported refuses, a negative or non-finite rtol / atol, min_niter < 0)"""
        t = self._sweep_target(rtol, atol, min_niter)
        return self._sweep_refusal(lambda p, a, why, n: lib().mci_sweep_until_supported(p, a, C.byref(t), why, n), solver, neval, niter, block, measurefreq)

    def integrate_sweep_until(self, solver="vegas", userdata=None, neval=10000, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0, measurefreq=1,
                              seed=1234, seeds=None, maps=None, first_iteration=0, rtol=0.0, atol=0.0, min_niter=0):
        """integrate_sweep with a target error (mci_integrate_sweep_until): every point runs until each of its statistics columns has
        E <= max(atol, rtol |M|) -- M, E the weighted average over its counted iterations and that average's error, as Result computes
        them --, from iteration max(ignore + 2, min_niter) on, and at most `niter` iterations; still ONE launch: a workgroup that has
        finished a point takes the next one nobody has begun.  Arguments and result dicts as integrate_sweep; every dict also carries
        `niter_run` (the iterations the point ran) and `converged` (whether it met the target: False when it ran all `niter` without), and
        its iter_mean / iter_std hold niter_run rows.  A point's results are those of integrate_sweep(..., niter=niter_run).  A column that
        is NaN or infinite never converges.  rtol = atol = 0 stops nothing early.  Raises MCIError with the reason of
        sweep_until_supported()."""
        ud, sd, mi, _ = self._sweep_inputs("integrate_sweep_until", userdata, seeds, maps)
        a = self._integrate_args(solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration)
        t = self._sweep_target(rtol, atol, min_niter)
        P = ud.shape[0]
        nrun = np.zeros(P, dtype=np.int32)
        fn = lambda p, a, P, ud, sd, mi, mo, res, im, ie, st: lib().mci_integrate_sweep_until(p, a, C.byref(t), P, ud, sd, mi, mo, res, im, ie, st,
                                                                                                 nrun.ctypes.data_as(c_int32_p))
        kept = {}
        out = self._sweep_call(fn, a, P, niter, (ud, sd, mi), lambda P: ((), {}), keep=kept)
        met = self._until_met(kept["iter_mean"], kept["iter_std"], nrun, ignore if ignore >= 0 else (1 if adapt else 0), t)
        for q, r in enumerate(out):
            n = int(nrun[q])
            r["niter_run"], r["converged"] = n, bool(met[q])
            r["iter_mean"], r["iter_std"] = r["iter_mean"][:n], r["iter_std"][:n]
        return out

    @staticmethod
    def _until_met(im, ie, nrun, ignore, t):
        """[P]: whether the rows each point came back with meet the target (the rule of csrc/mci_sweep_common.h on the host, all points
        at once), for the points that ran all niter iterations: such a point may have met the target in its last one.  A point that
        stopped below niter converged by definition -- the kernel's verdict, never second-guessed here.  im, ie: [P][niter][nobs], nrun [P]"""
        rows = np.arange(im.shape[1])[None, :, None]
        counted = (rows >= ignore) & (rows < nrun[:, None, None])
        with np.errstate(all="ignore"):
            w = np.where(counted, 1.0 / (ie + 1.0e-10) ** 2, 0.0)
            W = w.sum(1)
            M, E = np.where(counted, w * im, 0.0).sum(1) / W, 1.0 / np.sqrt(W)
            ok = np.isfinite(M) & np.isfinite(E) & (E <= np.maximum(t.atol, t.rtol * np.abs(M)))
        return (nrun < im.shape[1]) | (ok.all(1) & (nrun >= max(ignore + 2, t.min_niter)))

    def _sweep_inputs(self, name, userdata, seeds, maps, before_maps=None):
        """(userdata [P][nuserdata], seeds [P] | None, maps [P][sweep_map_doubles()] | None) as contiguous arrays, or the ValueError of
        entry point `name`; before_maps(): what the entry point checks between the seeds and the maps, its value the fourth of the tuple"""
        nud = len(self.integrand.userdata) if hasattr(self.integrand, "userdata") else 0
        ud = np.ascontiguousarray(userdata if userdata is not None else np.zeros((0, nud)), dtype=np.float64)
        if ud.ndim != 2 or ud.shape[1] != nud:
            raise ValueError("%s: userdata must be a 2-D array [points][%d] (one row of the integrand's userdata per point), got shape %s"
                             % (name, nud, ud.shape))
        P = ud.shape[0]
        if not 1 <= P <= self.SWEEP_MAX_POINTS:
            raise ValueError("%s: %d points; a sweep takes 1 to %d" % (name, P, self.SWEEP_MAX_POINTS))
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(seeds, dtype=np.uint64)
            if sd.shape != (P,):
                raise ValueError("%s: seeds must hold one seed per point (%d), got shape %s" % (name, P, sd.shape))
        between = before_maps() if before_maps else None
        nmap = self.sweep_map_doubles()
        mi = None
        if maps is not None:
            mi = np.ascontiguousarray(maps, dtype=np.float64)
            if mi.shape != (P, nmap):
                raise ValueError("%s: maps must be [points = %d][grid points = %d] (sweep_map_doubles(): every leaf's row, one behind the other), got shape %s"
                                 % (name, P, nmap, mi.shape))
        return ud, sd, mi, between

    def _sweep_call(self, fn, a, P, niter, arrays, extra, keep=None):
        """fn (mci_integrate_sweep | mci_integrate_sweep_strat | mci_integrate_sweep_chains | mci_integrate_sweep_mcmc) on the arrays of _sweep_inputs -> the list of P result dicts.  extra(P): the
        entry point's own arguments between maps_out and results, and the keys they add to every dict ({key: [P][...] array}); keep: a
        dict that is given the [P][niter][nobs] arrays the dicts' iter_mean / iter_std are rows of"""
        ud, sd, mi = arrays
        n, nmap = self.nobs, self.sweep_map_doubles()
        im, ie = np.zeros((P, niter, n)), np.zeros((P, niter, n))
        m, s, c2 = np.zeros((P, n)), np.zeros((P, n)), np.zeros((P, n))
        vis = np.zeros((P, self.config.N + 1))
        mo = np.zeros((P, max(nmap, 1)))
        own, keys = extra(P)
        st = np.zeros(P, dtype=np.int32)
        res = (_lib.ResultC * P)()
        for q in range(P):
            res[q] = _lib.ResultC(niter, n, None, None, _dp(m[q]), _dp(s[q]), _dp(c2[q]), 0, 0.0, _dp(vis[q]), 0, 0)
        check(fn(self.p, C.byref(a), P, _dp(ud) if ud.size else None, sd.ctypes.data_as(C.POINTER(C.c_uint64)) if sd is not None else None,
                 _dp(mi) if mi is not None else None, _dp(mo), *own, res, _dp(im), _dp(ie), st.ctypes.data_as(c_int32_p)))
        if keep is not None:
            keep.update(iter_mean=im, iter_std=ie)
        out = []
        for q in range(P):
            r = dict(mean=m[q], stdev=s[q], chi2=c2[q], iter_mean=im[q], iter_std=ie[q], neval=res[q].neval, seconds=res[q].seconds,
                     visited=vis[q], correlated=bool(res[q].correlated), block_mean=None, warmup=0, neval_discarded=0, maps=mo[q],
                     maps_by_leaf=self._split_sweep_map(mo[q]), status=int(st[q]))
            for k, v in keys.items():
                r[k] = v[q]
            out.append(r)
        return out

    def sweep_strat_supported(self, solver="vegas", neval=10000, niter=10, block=16, measurefreq=1, **kw):
        """None when integrate_sweep_strat takes this (stratified) problem with these arguments, else the reason
        (mci_sweep_strat_supported)"""
        return self._sweep_refusal(lib().mci_sweep_strat_supported, solver, neval, niter, block, measurefreq)

    def sweep_strat_geometry(self, neval=10000, block=16):
        """{chunk, lds_bytes, map_off, mblocks} of the launch integrate_sweep_strat lays these arguments out as: samples per chunk,
        dynamic LDS per workgroup, the map's place in it (doubles), the blocks the ordinary stratified call merges its rows as; see
        csrc/mci_debug.h mci_debug_sweep_strat_geometry (no device needed)"""
        a = self._integrate_args("vegas", neval, 1, block, -1, True, 1.0, 1, 0, 0)
        ch, lds, off, mb = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().mci_debug_sweep_strat_geometry(self.p, C.byref(a), C.byref(ch), C.byref(lds), C.byref(off), C.byref(mb)))
        return dict(chunk=int(ch.value), lds_bytes=int(lds.value), map_off=int(off.value), mblocks=int(mb.value))

    def sweep_strat_plan(self, neval=10000, block=16):
        """{nstrat, ncube, beta} of the plan a stratified sweep of these arguments runs on: the nstrat set_stratification was given, or
        the default plan for this neval (mci_strat_plan)"""
        req = getattr(self, "_strat_req", None)
        if req is None:
            raise ValueError("sweep_strat_plan: the problem is not stratified (set_stratification)")
        a = self._integrate_args("vegas", neval, 1, block, -1, True, 1.0, 1, 0, 0)
        nc = C.c_int64()
        check(lib().mci_sweep_strat_doubles(self.p, C.byref(a), C.byref(nc)))
        if req[0] is not None:
            ns = list(req[0])
        else:
            npb, nb = C.c_int64(), C.c_int64()
            lib().mci_standardize_block(int(neval), int(block), 1, C.byref(npb), C.byref(nb))
            buf = np.zeros(self.ndraw, dtype=np.int32)
            check(lib().mci_strat_plan(npb.value * nb.value, self.ndraw, req[2], buf.ctypes.data_as(c_int32_p)))
            ns = [int(v) for v in buf]
        return dict(nstrat=ns, ncube=int(nc.value), beta=req[1])

    def integrate_sweep_strat(self, solver="vegas", userdata=None, neval=10000, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0, measurefreq=1,
                              seed=1234, seeds=None, maps=None, first_iteration=0, d=None):
        """A stratified parameter sweep in one launch (mci_integrate_sweep_strat): P independent VEGAS+ loops -- what integrate() runs on
        this stratified engine -- one workgroup per point.  Arguments and result dicts as integrate_sweep (one Continuous leaf; after
        set_sweep_strat_leaves("all") several: `maps` rows then hold sweep_map_doubles() doubles, the leaves' grids in order, and
        `maps_by_leaf` gives them leaf by leaf); every
        dict gains `strat_d` (the d_h the point's last iteration measured, [ncube]) and `strat_counts` (n_h of the allocation that
        iteration used).  d: None (every point starts from a uniform allocation) or [P][ncube] d_h measured on exactly this plan and
        beta -- e.g. the strat_d of an earlier sweep; with adapt=False the allocation made from it stays for the whole call.  The
        engine's own map, logs and allocation are not touched.  Raises MCIError with the reason of sweep_strat_supported()."""
        def plan():
            a = self._integrate_args(solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration)
            nc = C.c_int64()
            check(lib().mci_sweep_strat_doubles(self.p, C.byref(a), C.byref(nc)))
            return a, int(nc.value)
        ud, sd, mi, (a, ncube) = self._sweep_inputs("integrate_sweep_strat", userdata, seeds, maps, before_maps=plan)
        P = ud.shape[0]
        di = None
        if d is not None:
            di = np.ascontiguousarray(d, dtype=np.float64)
            if di.shape != (P, ncube):
                raise ValueError("integrate_sweep_strat: d must be [points = %d][hypercubes = %d], got shape %s" % (P, ncube, di.shape))

        def extra(P):
            do, co = np.zeros((P, ncube)), np.zeros((P, ncube), dtype=np.int64)
            return (_dp(di) if di is not None else None, _dp(do), co.ctypes.data_as(C.POINTER(C.c_int64))), dict(strat_d=do, strat_counts=co)
        return self._sweep_call(lib().mci_integrate_sweep_strat, a, P, niter, (ud, sd, mi), extra)

    def sweep_chains_supported(self, solver="vegasmc", neval=10000, niter=10, block=16, measurefreq=1, nchain=1, first_iteration=0, **kw):
        """None when integrate_sweep_chains takes this problem with these arguments, else the reason (mci_sweep_chains_supported)"""
        return self._sweep_refusal(lib().mci_sweep_chains_supported, solver, neval, niter, block, measurefreq, nchain, first_iteration)

    def integrate_sweep_chains(self, solver="vegasmc", userdata=None, neval=10000, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0,
                               measurefreq=1, seed=1234, seeds=None, maps=None, first_iteration=0, nchain=1, reweight=None, carry=False, state=None, keep_state=True):
        """A parameter sweep under the default solver in one launch (mci_integrate_sweep_chains): P independent :vegasmc loops -- what
        integrate("vegasmc", nchain=nchain) runs on this engine with set_chain_carry(0) and one lane per chain -- one workgroup per
        point, the blocks of a point one after another.  Arguments and result dicts as integrate_sweep (any mix of Continuous and
        Discrete leaves); every dict gains `reweight` (the point's factors after its last doReweight!, [N + 1]), `propose` and `accept`
        (the tables of its last iteration, shaped like acceptance()).  reweight: None (every point starts from the engine's current
        factors) or [P][N + 1], e.g. the `reweight` of an earlier sweep.  nchain >= 1: chains per block.  The engine's own map, factors,
        packed buffer, logs and carried chains are not touched.  Raises MCIError with the reason of sweep_chains_supported().
        carry=True: this call runs with set_sweep_chain_carry(True) -- what integrate("vegasmc", nchain=nchain) runs with
        set_chain_carry(1); `correlated` and `stdev` are then integrate()'s (the block-lineage error); False: whatever
        set_sweep_chain_carry says (off by default).
        state: None or one ChainState per point, the `chain_state` of the dicts of the call before (mci_integrate_sweep_chains_resume):
        with maps=, reweight= and first_iteration = the states' iteration + 1 the points are what integrate("vegasmc", nchain=nchain,
        first_iteration=...) is on an engine with set_chain_carry(1) that has just run that call -- iteration 0 continues the stored
        chains (their count may differ from nchain) unless they ran on a never-refined map that has been refined since.  A state that
        does not fit (solver, blocks, layout, a gap in the iteration numbers), carry off or nchain = 1 raise MCIError by name.  With
        carried chains and nchain > 1 every dict has `chain_state` (else None) and `continued` (iteration 0 continued a state).
        keep_state=False: no states are copied out (`chain_state` None): block x nchain x (ndraw + 1) doubles per point less to read back."""
        a = self._integrate_args(solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration, nchain)
        return self._sweep_chain_solver("integrate_sweep_chains", lib().mci_integrate_sweep_chains, a, niter, userdata, seeds, maps, reweight, False, carry,
                                        state, lib().mci_integrate_sweep_chains_resume, keep_state)

    def sweep_chain_state_doubles(self, solver="vegasmc", neval=10000, niter=10, block=16, measurefreq=1, nchain=2, first_iteration=0, adapt=True, thermal_ratio=0.1):
        """(doubles of one point's chain state row, the record a call with these arguments and no state writes: a dict)
        (mci_sweep_chain_state_doubles); MCIError where the chain sweep refuses the arguments or nchain < 2"""
        a = self._integrate_args(solver, neval, niter, block, -1, adapt, 1.0, measurefreq, 1234, first_iteration, nchain, thermal_ratio)
        n, info = C.c_int64(), _lib.SweepChainInfo()
        check(lib().mci_sweep_chain_state_doubles(self.p, C.byref(a), C.byref(n), C.byref(info)))
        return n.value, {k: getattr(info, k) for k, _ in _lib.SweepChainInfo._fields_}

    def sweep_chain_state_supported(self, state=None, solver="vegasmc", neval=10000, niter=10, block=16, measurefreq=1, nchain=2, first_iteration=0,
                                    adapt=True, thermal_ratio=0.1):
        """(None, continues) when the chain sweep of `solver` takes these arguments together with `state` (a ChainState, or None: states
        only go out) -- continues: iteration 0 goes on from the stored chains --, else (the reason, False) (mci_sweep_chain_state_supported)"""
        a = self._integrate_args(solver, neval, niter, block, -1, adapt, 1.0, measurefreq, 1234, first_iteration, nchain, thermal_ratio)
        why, cont = C.create_string_buffer(512), C.c_int32()
        info = self._chain_info(state) if state is not None else None
        rc = lib().mci_sweep_chain_state_supported(self.p, C.byref(a), C.byref(info) if info is not None else None, why, len(why), C.byref(cont))
        return (None, bool(cont.value)) if rc == 0 else (why.value.decode(), False)

    @staticmethod
    def _chain_info(st):
        return _lib.SweepChainInfo(_lib.SOLVERS[st.solver], st.nd, st.ndraw, st.iteration, st.ntrain, 1 if st.adapted else 0, st.blocks, st.nchain)

    def _sweep_chain_solver(self, name, fn, a, niter, userdata, seeds, maps, reweight, holds, carry=False, state=None, fn_resume=None, keep_state=True):
        """what integrate_sweep_chains and integrate_sweep_mcmc share: the arrays, the reweight check, the per-point factors and tables;
        holds: the entry point also returns every point's holding-time histogram; carry: set_sweep_chain_carry(True) for this call;
        state, fn_resume: the points' chain states and the entry point that takes them and hands them out"""
        if carry and not self.sweep_chain_carry():
            self.set_sweep_chain_carry(True)
            try:
                return self._sweep_chain_solver(name, fn, a, niter, userdata, seeds, maps, reweight, holds, False, state, fn_resume, keep_state)
            finally:
                self.set_sweep_chain_carry(False)
        ud, sd, mi, _ = self._sweep_inputs(name, userdata, seeds, maps)
        P, nd = ud.shape[0], self.config.N + 1
        m = max(nd, len(self.config.var))
        ri = None
        if reweight is not None:
            ri = np.ascontiguousarray(reweight, dtype=np.float64)
            if ri.shape != (P, nd):
                raise ValueError("%s: reweight must be [points = %d][integrands + 1 = %d], got shape %s" % (name, P, nd, ri.shape))

        # chains that travel between calls: states go out of every carried call with more than one chain per block; a state that comes
        # in is the library's to accept or to refuse by name
        from .statistics import ChainState
        keeps = fn_resume is not None and keep_state and self.sweep_chain_carry() and a.nchain > 1
        s_in = s_out = rows_in = rows_out = None
        if state is not None:
            state = list(state)
            if len(state) != P or not all(isinstance(s, ChainState) for s in state):
                raise ValueError("%s: state must hold one ChainState per point (%d), the chain_state of an earlier call's results" % (name, P))
            if any(s.record() != state[0].record() for s in state):
                raise ValueError("%s: the points' chain states disagree with each other (%s)"
                                 % (name, ", ".join(sorted({str(s.record()) for s in state}))))
            if any(s.data.shape != (state[0].row_doubles(),) for s in state):
                raise ValueError("%s: a chain state's array does not hold the %d doubles of its record" % (name, state[0].row_doubles()))
            rows_in = np.ascontiguousarray(np.stack([s.data for s in state]), dtype=np.float64)
            s_in = _lib.SweepChainState(self._chain_info(state[0]), _dp(rows_in))
        if keeps:
            n = C.c_int64()
            check(lib().mci_sweep_chain_state_doubles(self.p, C.byref(a), C.byref(n), None))
            rows_out = np.zeros((P, n.value))
            s_out = _lib.SweepChainState(_lib.SweepChainInfo(), _dp(rows_out))
        resume = s_in is not None or s_out is not None

        def extra(P):
            ro, pa = np.zeros((P, nd)), np.zeros((P, 2, 3, nd, m))
            own, keys = (_dp(ri) if ri is not None else None, _dp(ro), _dp(pa)), dict(reweight=ro, propose=pa[:, 0], accept=pa[:, 1])
            if holds:
                ho = np.zeros((P, 64), dtype=np.uint64)
                own += (ho.ctypes.data_as(C.POINTER(C.c_uint64)),)
                keys["holds"] = ho
            if resume:
                own += (C.byref(s_in) if s_in is not None else None, C.byref(s_out) if s_out is not None else None)
            return own, keys
        continued = False
        if s_in is not None:   # (asked before the call: the refusal by name, and whether iteration 0 goes on from the states)
            cont = C.c_int32()
            check(lib().mci_sweep_chain_state_supported(self.p, C.byref(a), C.byref(s_in.info), None, 0, C.byref(cont)))
            continued = bool(cont.value)
        out = self._sweep_call(fn_resume if resume else fn, a, P, niter, (ud, sd, mi), extra)
        for q, r in enumerate(out):
            r["continued"] = continued
            r["chain_state"] = None
            if s_out is not None:
                i = s_out.info
                r["chain_state"] = ChainState(_lib.SOLVER_NAMES[i.solver], i.blocks, i.nchain, i.ndraw, i.nd, i.iteration, i.ntrain, bool(i.adapted), rows_out[q].copy())
        if holds:
            for r in out:
                r["hold_max"] = self.hold_max_of(r["holds"])
        return out

    @staticmethod
    def hold_max_of(holds):
        """the upper bound 2^b - 1 of the highest occupied bin b of a holding-time histogram (hold_histogram's bins), 0 if none"""
        top = np.flatnonzero(np.asarray(holds))
        return (1 << int(top[-1])) - 1 if top.size else 0

    def sweep_mcmc_supported(self, solver="mcmc", neval=10000, niter=10, block=16, measurefreq=1, nchain=1, first_iteration=0, thermal_ratio=0.1, **kw):
        """None when integrate_sweep_mcmc takes this problem with these arguments, else the reason (mci_sweep_mcmc_supported)"""
        return self._sweep_refusal(lib().mci_sweep_mcmc_supported, solver, neval, niter, block, measurefreq, nchain, first_iteration, thermal_ratio)

    def integrate_sweep_mcmc(self, solver="mcmc", userdata=None, neval=10000, niter=10, block=16, ignore=-1, adapt=True, gamma=1.0,
                             measurefreq=1, seed=1234, seeds=None, maps=None, first_iteration=0, nchain=1, reweight=None, thermal_ratio=0.1, carry=False,
                             state=None, keep_state=True):
        """A parameter sweep under :mcmc in one launch (mci_integrate_sweep_mcmc): P independent :mcmc loops -- what
        integrate("mcmc", nchain=nchain, thermal_ratio=thermal_ratio) runs on this engine with set_chain_carry(0) and one lane per
        chain -- one workgroup per point, the blocks of a point one after another.  Arguments and result dicts as
        integrate_sweep_chains; every dict also carries `holds` (the point's holding-time histogram, 64 counts summed over the call's
        iterations and blocks: hold_histogram's bins) and `hold_max` (the upper bound 2^b - 1 of its highest occupied bin b, 0 if
        none).  There is no warm-up repetition and no automatic chain count: nchain >= 1 is explicit.  The engine's own map, factors,
        packed buffer, hold histogram, logs and carried chains are not touched.  Raises MCIError with the reason of sweep_mcmc_supported().
        carry=True: as in integrate_sweep_chains -- every iteration after a point's first continues the stored chains, resampled to the
        moved reweight factors, with no burn-in; every dict's `carried` says whether the point's later iterations were.
        state: as in integrate_sweep_chains (mci_integrate_sweep_mcmc_resume) -- iteration 0 of a call with states that fit always
        continues the stored chains, so no iteration of the call holds a burn-in; `chain_state`, `continued` and keep_state as there."""
        a = self._integrate_args(solver, neval, niter, block, ignore, adapt, gamma, measurefreq, seed, first_iteration, nchain, thermal_ratio)
        out = self._sweep_chain_solver("integrate_sweep_mcmc", lib().mci_integrate_sweep_mcmc, a, niter, userdata, seeds, maps, reweight, True, carry,
                                       state, lib().mci_integrate_sweep_mcmc_resume, keep_state)
        for r in out:
            r["carried"] = bool((carry or self.sweep_chain_carry()) and nchain > 1 and (niter > 1 or r["continued"]))
        return out

    def sweep_workgroups(self, g=0):
        """test hook of csrc/mci_debug.h: workgroups of the next sweeps (0 = the default), so that one workgroup runs several points"""
        check(lib().mci_debug_sweep_workgroups(self.p, int(g)))

    def sweep_threads(self, threads=0):
        """A/B hook of csrc/mci_debug.h: threads per workgroup of the next sweeps (256 | 512 | 1024; 0 = the default)"""
        check(lib().mci_debug_sweep_threads(self.p, int(threads)))

    def last_sweep_launch(self):
        """(workgroups, threads per workgroup) of the last sweep launch"""
        g, t = C.c_int32(), C.c_int32()
        check(lib().mci_debug_sweep_last_launch(self.p, C.byref(g), C.byref(t)))
        return int(g.value), int(t.value)

    def sweep_lds_bytes(self):
        """LDS bytes a workgroup of this problem's sweeps takes (csrc/mci_debug.h; tools/sweep_bench.py)"""
        n = C.c_int64()
        check(lib().mci_debug_sweep_lds_bytes(self.p, C.byref(n)))
        return int(n.value)

    def mcmc_launch_valid(self):
        """(the last automatic :mcmc launch was long enough for the holds it measured, some launch of this problem has been, its chain
        length, its longest hold); waits for that launch's sample kernel -- see mci_mcmc_launch_valid"""
        v, w, ln, h = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        check(lib().mci_mcmc_launch_valid(self.p, C.byref(v), C.byref(w), C.byref(ln), C.byref(h)))
        return bool(v.value), bool(w.value), int(ln.value), int(h.value)

    def discard_iteration(self):
        """the last finished iteration out of the iteration log and the block log again (a warm-up launch that is run again)"""
        check(lib().mci_iteration_discard(self.p))

    def block_means(self, rows):
        """chain solvers: (block means [rows][local blocks][nobs] of the last `rows` iterations, how many of the logged iterations
        continued the chains of the one before); see mci_get_block_means"""
        nb, carried = C.c_int64(), C.c_int32()
        check(lib().mci_get_block_means(self.p, 0, None, C.byref(nb), C.byref(carried)))
        out = np.zeros((int(rows), int(nb.value), self.nobs))
        if rows > 0 and out.size:
            check(lib().mci_get_block_means(self.p, int(rows), _dp(out), C.byref(nb), C.byref(carried)))
        return out, int(carried.value)

    def comm_sum(self, v):
        """v summed over the ranks of the library's communicator (mci_comm_sum)"""
        a = np.ascontiguousarray(v, dtype=np.float64).copy()
        check(lib().mci_comm_sum(self.p, _dp(a), a.size))
        return a

    def reset_block_log(self):
        check(lib().mci_reset_block_log(self.p))

    def comm_ranks(self):
        """ranks of the communicator attached to this engine's context (1: none; mci_integrate shards its blocks over them)"""
        r, n = C.c_int32(), C.c_int32()
        check(lib().mci_comm_rank(context(self.device), C.byref(r), C.byref(n)))
        return int(n.value)

    # ---- stratified :vegas (VEGAS+; mci_set_stratification) ---------------------------------------------------------------------
    CARRIED = ("uniform", "same plan", "remapped")   # mci_get_strat_carry: where the last first-allocation of a run came from

    def set_stratification(self, nstrat=None, beta=0.75, max_nhcube=2 ** 24, on=True, carry=False):
        """stratified :vegas from the next iteration on (nstrat None: the default plan for the iteration's neval, mci_strat_plan);
        on=False: back to plain :vegas.  carry=True (mci_set_stratification_carry): the d_h of the last finished iteration, or of a
        loaded state file, stays with the engine -- through this setter too -- and the next call's first allocation is made from it"""
        if not on:
            check(lib().mci_set_stratification_off(self.p))
            self._strat_req = None
            return
        self._strat_req = (None if nstrat is None else [int(v) for v in np.atleast_1d(nstrat)], float(beta), int(max_nhcube))
        check(lib().mci_set_stratification_carry(self.p, 1 if carry else 0))   # (first: the setter below keeps a carried d_h only then)
        ns = None
        if nstrat is not None:
            self._nstrat = np.ascontiguousarray(nstrat, dtype=np.int32)
            ns = self._nstrat.ctypes.data_as(c_int32_p)
        check(lib().mci_set_stratification(self.p, self.ndraw, ns, float(beta), int(max_nhcube)))

    def stratification(self):
        """{nstrat, ncube, beta} of the plan in use, None when the problem is not stratified; an engine that carries its allocation
        (set_stratification(carry=True)) adds carry = True and carried = "uniform" | "same plan" | "remapped": where the first
        allocation of its last run came from"""
        ns, nc, b = np.zeros(self.ndraw, dtype=np.int32), C.c_int64(), C.c_double()
        check(lib().mci_get_stratification(self.p, ns.ctypes.data_as(c_int32_p), C.byref(nc), C.byref(b)))
        if not ns.any():
            return None
        info = dict(nstrat=[int(v) for v in ns], ncube=int(nc.value), beta=float(b.value))
        on, how = self.strat_carry()
        if on:
            info.update(carry=True, carried=self.CARRIED[how])
        return info

    def strat_carry(self):
        """(carry on?, how the last first-allocation started: 0 uniform | 1 the carried d_h on its own plan | 2 remapped)"""
        on, how = C.c_int32(), C.c_int32()
        check(lib().mci_get_strat_carry(self.p, C.byref(on), C.byref(how)))
        return bool(on.value), int(how.value)

    def strat_start_d_next(self, n):
        """test hook (mci_debug_strat_start_d): buffer the next first-allocation of a run fills with the n = ncube d_h it is made from"""
        self._strat_start_d = np.zeros(int(n))
        check(lib().mci_debug_strat_start_d(self.p, _dp(self._strat_start_d), int(n)))
        return self._strat_start_d

    def strat_counts(self):
        """n_h of every hypercube in the allocation the last stratified iteration used"""
        info = self.stratification()
        n = info["ncube"] if info else 0
        out = np.zeros(n, dtype=np.int64)
        check(lib().mci_get_strat_counts(self.p, out.ctypes.data_as(C.POINTER(C.c_int64)), n))
        return out

    def strat_d(self):
        """test hook (mci_debug_strat_d): the damped weights d_h the last finished stratified iteration wrote"""
        info = self.stratification()
        out = np.zeros(info["ncube"] if info else 0)
        check(lib().mci_debug_strat_d(self.p, _dp(out), out.size))
        return out

    def strat_dump_next(self, n):
        """test hook (mci_debug_strat_dump): buffers the next stratified iteration of n samples fills -- x, y [n, ndraw], h [n], jac [n],
        w [n, N * ncomp]; read them after that iteration ran"""
        d = dict(x=np.zeros((n, self.ndraw)), y=np.zeros((n, self.ndraw)), h=np.zeros(n, dtype=np.int64), jac=np.zeros(n),
                 w=np.zeros((n, self.config.N * self.config.ncomp)))
        self._strat_dump = d
        check(lib().mci_debug_strat_dump(self.p, int(n), _dp(d["x"]), _dp(d["y"]), d["h"].ctypes.data_as(C.POINTER(C.c_int64)),
                                         _dp(d["jac"]), _dp(d["w"])))
        return d

    def sample_dump(self, n, nevalperblock=None, block_index=0, iteration=0, seed=1234):
        nevalperblock = n if nevalperblock is None else nevalperblock
        x, jac, w = np.empty((n, self.ndraw)), np.empty(n), np.empty((n, self.config.N * self.config.ncomp))
        check(lib().mci_sample_dump(self.p, iteration, seed, int(nevalperblock), int(block_index), int(n), _dp(x), _dp(jac), _dp(w)))
        return x, jac, w

    def kernel_times_ms(self, n=512):
        """HIP-event durations of the last n sampling-kernel launches (oldest first), (workgroups, threads)"""
        ms = (C.c_float * n)()
        got, wg, th = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().mci_kernel_times_ms(self.p, ms, n, C.byref(got), C.byref(wg), C.byref(th)))
        return np.array(ms[:got.value], dtype=np.float64), wg.value, th.value

    def kernel_clocks_mhz(self, n=512):
        """shader clock (MHz) of the last n timed :vegas launches, from s_memtime / s_memrealtime around the sample loop; see mci_kernel_clocks"""
        out = np.empty(n)
        got = C.c_int32()
        check(lib().mci_kernel_clocks(self.p, _dp(out), n, C.byref(got)))
        return out[:got.value].copy()

    def comm_times_ms(self, n=64):
        """HIP-event durations of this rank's last n per-iteration all-reduces inside the library (oldest first; recorded under the
        sample launch's timing rule, set_kernel_timing)"""
        ms = (C.c_float * n)()
        got = C.c_int32()
        check(lib().mci_comm_times_ms(self.p, ms, n, C.byref(got)))
        return np.array(ms[:got.value], dtype=np.float64)

    def last_kernel_ms(self):
        ms, wg, th = self.kernel_times_ms(1)
        return (float(ms[-1]) if len(ms) else float("nan")), wg, th   # (nan: the launch ran without events, set_kernel_timing)

    # ---- state ---------------------------------------------------------------------------------
    def grid(self, leaf):
        n = self.config.leaves[leaf].ninc
        out = np.empty(n)
        check(lib().mci_get_grid(self.p, leaf, _dp(out), n))
        return out

    def set_grid(self, leaf, grid):
        g = np.ascontiguousarray(grid, dtype=np.float64)
        check(lib().mci_set_grid(self.p, leaf, _dp(g), len(g)))

    def distribution(self, leaf):
        lf = self.config.leaves[leaf]
        k = lf.upper - lf.lower + 1
        d, a = np.empty(k), np.empty(k + 1)
        check(lib().mci_get_distribution(self.p, leaf, _dp(d), _dp(a), k))
        return d, a

    def set_distribution(self, leaf, dist):
        d = np.ascontiguousarray(dist, dtype=np.float64)
        check(lib().mci_set_distribution(self.p, leaf, _dp(d), len(d)))

    def histogram(self, leaf):
        """histogram section of the packed buffer for one leaf"""
        packed = self.get_packed()
        off = 2 * self.nobs + 2 + self.config.N + 1
        for i, lf in enumerate(self.config.leaves):
            nb = (lf.ninc - 1) if isinstance(lf, ContinuousVar) else 1 if isinstance(lf, FermiK) else (lf.upper - lf.lower + 1)
            if i == leaf:
                return packed[off:off + nb]
            off += nb
        raise IndexError(leaf)

    def reweight(self):
        out = np.empty(self.config.N + 1)
        check(lib().mci_get_reweight(self.p, _dp(out), len(out)))
        return out

    def acceptance(self):
        """(propose, accept) of the last iteration, each shaped [3, N+1, max(N+1, Nv)] like config.propose / config.accept
        (configuration.jl:185-186; 0-based: [update, integrand, target]); see mci_get_acceptance"""
        nd = self.config.N + 1
        m = max(nd, len(self.config.var))
        n = 3 * nd * m
        pr, ac = np.empty(n), np.empty(n)
        check(lib().mci_get_acceptance(self.p, _dp(pr), _dp(ac), n))
        return pr.reshape(3, nd, m), ac.reshape(3, nd, m)

    def histograms(self):
        """histogram section of the packed buffer (all leaves, concatenated)"""
        off = 2 * self.nobs + 2 + self.config.N + 1
        nd = self.config.N + 1
        npa = 3 * nd * max(nd, len(self.config.var))
        return self.get_packed()[off:self.packed_size - 2 * npa]

    def set_reweight_goal(self, goal):
        if goal is None:
            check(lib().mci_set_reweight_goal(self.p, None, 0))
        else:
            g = np.ascontiguousarray(goal, dtype=np.float64)
            check(lib().mci_set_reweight_goal(self.p, _dp(g), len(g)))

    def set_reweight(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        check(lib().mci_set_reweight(self.p, _dp(r), len(r)))
