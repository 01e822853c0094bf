"""The constant optimiser's state machine on the host (csrc/srhip_bfgs.cpp through srhip_bfgs_host; no
device): Optim's BFGS / one-constant Newton over BackTracking, best of the starts, and the scheduling on
top of it (value-only trials, speculative trial points), against oracle/optim.py.

The callback evaluates closed-form objectives in Python floats and the same Python functions are handed
to optim.bfgs_exact / optim.newton_exact, so both sides see identical objective and gradient bits; every
comparison is exact (== on floats).  A non-finite objective value counts as +Inf on both sides, as the
callback contract says.  Every objective's calls are logged, and each case asserts from the logs that the
path it is there for was taken."""
import ctypes
import math

import numpy as np
import pytest

import optim
import srhip._lib as L

CBRT_EPS = 6.055454452393343e-06  # the Newton probes' step: cbrt(eps(Float64)) max(1, |c|)


class Objective:
    """f and its gradient over Python floats; `log` records every call of either side in order:
    ("f", x, value) and ("g", x, gradient)."""

    def __init__(self, n, f, grad):
        self.n, self._f, self._grad, self.log = n, f, grad, []

    def f(self, x):
        x = tuple(float(v) for v in x)
        try:
            v = float(self._f(*x))
        except (OverflowError, ValueError, ZeroDivisionError):
            v = math.inf
        if not math.isfinite(v):
            v = math.inf  # the callback contract: finite or +Inf
        self.log.append(("f", x, v))
        return v

    def grad(self, x):
        x = tuple(float(v) for v in x)
        try:
            g = tuple(float(v) for v in self._grad(*x))
        except (OverflowError, ValueError, ZeroDivisionError):
            g = (math.nan,) * self.n  # (a Hessian probe beyond a wall: the machine must not use it)
        self.log.append(("g", x, g))
        return list(g)


def _rosen(n):
    def f(*x):
        return sum(100.0 * (x[i + 1] - x[i] * x[i]) ** 2 + (1.0 - x[i]) ** 2 for i in range(n - 1))

    def g(*x):
        out = [0.0] * n
        for i in range(n - 1):
            out[i] += -400.0 * x[i] * (x[i + 1] - x[i] * x[i]) - 2.0 * (1.0 - x[i])
            out[i + 1] += 200.0 * (x[i + 1] - x[i] * x[i])
        return out

    return Objective(n, f, g)


def _quartic(n, K, w):
    """sum x_i^4 + K sum w_i x_i^2"""
    return Objective(n, lambda *x: sum(v ** 4 for v in x) + K * sum(wi * v * v for wi, v in zip(w, x)),
                     lambda *x: [4.0 * v ** 3 + 2.0 * K * wi * v for wi, v in zip(w, x)])


def _wall_f(a, b):  # not finite for 1 < a + b < 3; the first search from (0, 0) overshoots, then lands inside twice
    r = a + b
    return 2.5 * (r - 2.5) ** 2 - math.log((r - 1.0) * (r - 3.0))


def _wall_g(a, b):
    r = a + b
    d = 5.0 * (r - 2.5) - (2.0 * r - 4.0) / ((r - 1.0) * (r - 3.0))
    return [d, d]


def _symmetric():  # f(a, b) = f(-a, b), in every rounding: mirrored starts tie bit for bit
    return Objective(2, lambda a, b: (a * a - 1.0) ** 2 + (b - 0.5) ** 2 + 0.25 * a * a * b * b,
                     lambda a, b: [4.0 * a * (a * a - 1.0) + 0.5 * a * b * b, 2.0 * (b - 0.5) + 0.5 * a * a * b])


# name -> (objective factory, start, iterations)
CASES = {
    "rosenbrock": (lambda: _rosen(2), (-1.2, 1.0), 8),
    # the Hessian at the start is ~ 2e100 diag(-1.1, 1.2, 0.3); a step across the quartic's valley has
    # dg'H dg overflow, the update leaves H non-finite, and the next direction is no descent direction
    "quartic3_indefinite": (lambda: _quartic(3, 1e100, (-1.1, 1.2, 0.3)), (-7.3e41, -1.2e43, -4e40), 8),
    "exp_overflow": (lambda: Objective(2, lambda a, b: math.exp(20.0 * a + 20.0 * b) - 1000.0 * (a + b),
                                       lambda a, b: [20.0 * math.exp(20.0 * a + 20.0 * b) - 1000.0] * 2),
                     (0.0, 0.0), 8),
    "log_wall": (lambda: Objective(2, _wall_f, _wall_g), (0.0, 0.0), 8),
    "slope_neginf": (lambda: Objective(2, lambda a, b: math.atan(1e200 * a) + math.atan(1e200 * b),
                                       lambda a, b: [1e200 / (1.0 + (1e200 * a) ** 2), 1e200 / (1.0 + (1e200 * b) ** 2)]),
                     (0.0, 0.0), 8),
    "newton_negative_curvature": (lambda: Objective(1, lambda x: x ** 4 - 2.0 * x * x, lambda x: [4.0 * x ** 3 - 4.0 * x]),
                                  (0.3,), 8),
    "newton_linear": (lambda: Objective(1, lambda x: 3.0 * x + 1.0, lambda x: [3.0]), (0.5,), 8),
    "newton_probe_nonfinite": (lambda: Objective(1, lambda x: x - math.log(x), lambda x: [1.0 - 1.0 / x]), (1e-6,), 8),
    "start_converged": (lambda: Objective(2, lambda a, b: (a - 1.0) ** 2 + (b + 2.0) ** 2,
                                          lambda a, b: [2.0 * (a - 1.0), 2.0 * (b + 2.0)]), (1.0, -2.0), 8),
    "start_nonfinite": (lambda: Objective(2, lambda a, b: math.log(a + b), lambda a, b: [1.0 / (a + b)] * 2),
                        (-1.0, -1.0), 8),
    "newton_start_nonfinite": (lambda: Objective(1, lambda x: math.log(x), lambda x: [1.0 / x]), (-1.0,), 8),
    "no_iterations": (lambda: _rosen(2), (-1.2, 1.0), 0),
    "newton_no_iterations": (lambda: Objective(1, lambda x: x ** 4 - 2.0 * x * x, lambda x: [4.0 * x ** 3 - 4.0 * x]),
                             (0.3,), 0),
}


class HostRun:
    """One srhip_bfgs_host call over `objs` (one tree each, trees without constants allowed as None).
    items: every item the callback was given, (call, tree, x, value_only, speculative, f) -- an item is
    speculative when its tree already had an item in the same call."""

    def __init__(self, objs, starts, iterations=8, g_tol=0.0, value_trials=1, spec_slots=32, spec_max_active=64,
                 spec_max_depth=64, fail_at=None, fail_code=7):
        n = [0 if o is None else o.n for o in objs]
        coff = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, int(coff[-1]))
        self.items, self.ncalls = [], 0

        def cb(_user, nitems, tree, x_off, x, value_only, f, g):
            if fail_at is not None and self.ncalls == fail_at:
                return fail_code
            seen = set()
            for i in range(nitems):
                t, o = tree[i], x_off[i]
                xs = tuple(x[o + k] for k in range(n[t]))
                f[i] = objs[t].f(xs)
                if not value_only[i]:
                    for k, gv in enumerate(objs[t].grad(xs)):
                        g[o + k] = gv
                self.items.append((self.ncalls, t, xs, int(value_only[i]), t in seen, f[i]))
                seen.add(t)
            self.ncalls += 1
            return 0

        q = L.BfgsQuery(ntrees=len(objs), nstarts=st.shape[0], const_offsets=coff.ctypes.data, starts=st.ctypes.data,
                        iterations=iterations, value_trials=value_trials, spec_slots=spec_slots,
                        spec_max_active=spec_max_active, spec_max_depth=spec_max_depth, g_tol=g_tol)
        self.best_x = np.full(int(coff[-1]), -77.0)
        self.best_f = np.full(len(objs), -77.0)
        self.fcalls = np.full(len(objs), -77, np.int64)
        nl = ctypes.c_int64(-77)
        self.rc = L.load().srhip_bfgs_host(ctypes.byref(q), L.BFGS_EVAL_FN(cb), None, L.ptr(self.best_x), L.ptr(self.best_f),
                                           L.ptr(self.fcalls), ctypes.byref(nl))
        self.nlaunches = nl.value
        self.coff = coff

    def result(self, t):
        return tuple(self.best_x[self.coff[t]:self.coff[t + 1]]), float(self.best_f[t]), int(self.fcalls[t])

    def results(self):
        return [self.result(t) for t in range(len(self.best_f))]


def oracle_start(obj, x0, iterations):
    """(x, f, calls) of one start by oracle/optim.py"""
    algorithm = optim.newton_exact if obj.n == 1 else optim.bfgs_exact
    x, fx, calls = algorithm(obj.f, obj.grad, np.asarray(x0, dtype=np.float64), iterations)
    return tuple(float(v) for v in x), float(fx), int(calls)


def oracle_best(obj, starts, iterations):
    """optimize_constants_exact's best-of loop over the starts (its lines 381-388)"""
    best_x, best_f, calls = None, np.inf, 0
    for s, xs in enumerate(starts):
        xr, fr, c = oracle_start(obj, xs, iterations)
        calls += c
        if s == 0 or fr < best_f:
            best_x, best_f = xr, fr
    return best_x, best_f, calls


def parse_log(log, n):
    """One start's oracle log, in the machine's terms: probes (points), searches (each line search's
    trials as (x, f)), accepted (the points a gradient was asked for after a search)."""
    out = dict(probes=[], searches=[], accepted=[], gradients=[])
    i = 0
    assert log[0][0] == "f"
    i = 1
    if i < len(log) and log[i][0] == "g":
        out["gradients"].append(log[i])
        x = log[i][1]
        i += 1
    while i < len(log):
        if n == 1 and log[i][0] == "f":
            e = CBRT_EPS * max(1.0, abs(x[0]))
            if log[i][1] == (x[0] + e,) and i + 1 < len(log) and log[i + 1][1] == (x[0] - e,):
                out["probes"] += [log[i], log[i + 1]]
                i += 2
                if i + 1 < len(log) and log[i][0] == "g" and log[i][1] == (x[0] + e,):
                    i += 2
        trials = []
        while i < len(log) and log[i][0] == "f":
            trials.append((log[i][1], log[i][2]))
            i += 1
        if trials:
            out["searches"].append(trials)
        if i < len(log):
            assert log[i][0] == "g"
            out["gradients"].append(log[i])
            out["accepted"].append(log[i][1])
            x = log[i][1]
            i += 1
    return out


def run_case(name, **kw):
    make, x0, iterations = CASES[name]
    ho, oo = make(), make()
    host = HostRun([ho], [x0], iterations=iterations, **kw)
    assert host.rc == 0
    want = oracle_start(oo, x0, iterations)
    return host, want, parse_log(oo.log, oo.n), ho, oo


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_start_equals_oracle(name):
    """best_x, best_f and fcalls of one start equal optim.bfgs_exact / newton_exact bit for bit; and run
    sequentially (no value-only trials, no speculation) the callback is given the oracle's own sequence of
    objective points."""
    host, want, _, _, oo = run_case(name)
    assert host.result(0) == want
    seq, want2, _, _, _ = run_case(name, value_trials=0, spec_slots=0)
    assert seq.result(0) == want == want2
    assert not any(it[3] or it[4] for it in seq.items)
    points = [e[1] for e in oo.log if e[0] == "f"]
    given = [it[2] for it in seq.items]
    if name == "slope_neginf":  # the machine counts the trials that must fail without launching them
        assert len(given) == 2 and len(points) == 1002
    else:
        assert len(given) == len(points)
    assert given == points[:len(given)]


def test_named_paths_are_taken():
    """Each case of test_one_start_equals_oracle takes the path it is named for (from the call logs)."""
    # Rosenbrock: eight full iterations, every update applied
    host, want, p, _, _ = run_case("rosenbrock")
    assert len(p["searches"]) == 8 and len(p["accepted"]) == 8 and want[2] == 1 + sum(map(len, p["searches"]))

    # the indefinite quartic: an update skipped (dx'dg <= 0), and after an applied update a direction that is
    # no descent direction (dphi0 >= 0 or NaN): the search then starts at x - g exactly, as only H = I gives
    host, want, p, _, _ = run_case("quartic3_indefinite")
    gs = p["gradients"]
    dxdg = [sum((a - b) * (c - d) for a, b, c, d in zip(gs[k][1], gs[k - 1][1], gs[k][2], gs[k - 1][2]))
            for k in range(1, len(gs))]
    assert any(d <= 0.0 for d in dxdg), dxdg
    resets = [k for k in range(1, len(gs) - 1)
              if any(d > 0.0 for d in dxdg[:k]) and p["searches"][k][0][0] == tuple(x - g for x, g in zip(gs[k][1], gs[k][2]))]
    assert resets, "no steepest-descent reset after an applied update"

    # exp: the first trial overflows; alpha is halved until the value is finite, then Armijo shrinks it on
    host, want, p, _, _ = run_case("exp_overflow")
    first = [v for _, v in p["searches"][0]]
    k = next(i for i, v in enumerate(first) if math.isfinite(v))
    assert k >= 2 and all(v == math.inf for v in first[:k]) and len(first) > k + 1
    alphas = [x[0] / p["searches"][0][0][0][0] for x, _ in p["searches"][0]]
    assert alphas[:k + 1] == [0.5 ** i for i in range(k + 1)]  # halving, exactly

    # the wall: a finite trial fails Armijo and the next, interpolated one is not finite
    host, want, p, _, _ = run_case("log_wall")
    v = [val for _, val in p["searches"][0]]
    assert math.isfinite(v[0]) and v[1] == v[2] == math.inf and math.isfinite(v[-1]) and len(p["accepted"]) >= 1

    # g's = -Inf: 1 + 1 + 1000 calls counted, two of them launched
    host, want, p, ho, _ = run_case("slope_neginf")
    assert want == ((0.0, 0.0), 0.0, 1002) and len(p["searches"]) == 1 and len(p["searches"][0]) == 1001
    assert host.nlaunches <= 3 and sum(1 for it in host.items if not it[4]) == 2

    # Newton: the curvature the probes see at the start
    for name, check in (("newton_negative_curvature", lambda h: h < 0.0), ("newton_linear", lambda h: h == 0.0)):
        host, want, p, _, oo = run_case(name)
        x0 = CASES[name][1][0]
        e = CBRT_EPS * max(1.0, abs(x0))
        assert [q[1] for q in p["probes"][:2]] == [(x0 + e,), (x0 - e,)]
        h = (oo._grad(x0 + e)[0] - oo._grad(x0 - e)[0]) / (2.0 * e)
        assert check(h), (name, h)
        assert [it[2] for it in host.items[1:3]] == [(x0 + e,), (x0 - e,)] and want[2] > 1
    host, want, p, _, _ = run_case("newton_probe_nonfinite")
    assert math.isfinite(p["probes"][0][2]) and p["probes"][1][2] == math.inf and want[2] > 1
    # ... with |h| = 1 the first trial is x - g
    x0 = CASES["newton_probe_nonfinite"][1][0]
    assert p["searches"][0][0][0] == (x0 - (1.0 - 1.0 / x0),)

    # one call each: a start at a minimum, a start where f is not finite, no iterations
    for name in ("start_converged", "start_nonfinite", "newton_start_nonfinite", "no_iterations", "newton_no_iterations"):
        host, want, p, _, _ = run_case(name)
        assert want[2] == 1 and host.nlaunches == 1 and len(host.items) == 1 and want[0] == CASES[name][1], name
    assert run_case("start_nonfinite")[1][1] == math.inf and run_case("start_converged")[1][1] == 0.0


def test_best_of_several_starts():
    """The first start's result is kept unconditionally, a later one replaces it only if strictly smaller:
    optimize_constants_exact's loop over the same bfgs_exact / newton_exact.  The mirrored starts tie bit
    for bit; the first start of `worse_first` ends non-finite and is still the result until a later start
    beats it."""
    cases = [
        (_symmetric, [(0.5, 0.3), (-0.5, 0.3), (0.5, 0.3)]),          # a tie: the first stays
        (_symmetric, [(-0.5, 0.3), (0.5, 0.3)]),                       # ... whichever it is
        (_symmetric, [(2.0, 2.0), (0.5, 0.3), (3.0, -1.0)]),           # a later start strictly smaller
        (lambda: _rosen(2), [(-1.2, 1.0), (0.0, 0.0), (2.0, 2.0)]),
        (CASES["start_nonfinite"][0], [(-1.0, -1.0), (-2.0, -1.0)]),   # every start +Inf: the first start's point
        (CASES["start_nonfinite"][0], [(-1.0, -1.0), (2.0, 1.0)]),
        (CASES["newton_negative_curvature"][0], [(0.3,), (-0.3,), (1.5,)]),
    ]
    for make, starts in cases:
        host = HostRun([make()], starts)
        assert host.rc == 0
        assert host.result(0) == oracle_best(make(), starts, 8), starts
    a, b = oracle_start(_symmetric(), (0.5, 0.3), 8), oracle_start(_symmetric(), (-0.5, 0.3), 8)
    assert a[1] == b[1] and a[0] == (-b[0][0], b[0][1]) and a[0][0] != 0.0  # the tie is one, with distinct points
    assert HostRun([_symmetric()], [(0.5, 0.3), (-0.5, 0.3)]).result(0)[0] == a[0]


def _batch():
    """Twelve trees with 1, 2, 3 and 5 constants, two starts each (the second a perturbed copy)."""
    makers = [
        CASES["newton_negative_curvature"][0], CASES["rosenbrock"][0], CASES["quartic3_indefinite"][0], lambda: _rosen(5),
        CASES["newton_linear"][0], CASES["exp_overflow"][0], lambda: _rosen(3), lambda: _quartic(5, 3.0, (-1.0, 2.0, -0.5, 0.25, 1.0)),
        CASES["newton_probe_nonfinite"][0], CASES["log_wall"][0], lambda: _quartic(3, 2.0, (-1.0, 0.5, -2.0)),
        lambda: Objective(5, lambda *x: math.exp(sum(3.0 * v for v in x)) + sum(v * v for v in x),
                          lambda *x: [3.0 * math.exp(sum(3.0 * v for v in x)) + 2.0 * v for v in x]),
    ]
    x0 = [CASES["newton_negative_curvature"][1], CASES["rosenbrock"][1], CASES["quartic3_indefinite"][1],
          (-1.2, 1.0, -0.5, 0.8, 1.1), CASES["newton_linear"][1], CASES["exp_overflow"][1], (-1.2, 1.0, 0.7),
          (0.3, -0.2, 0.1, 1.5, -0.7), CASES["newton_probe_nonfinite"][1], CASES["log_wall"][1], (0.2, -0.1, 0.3),
          (1.0, 2.0, -0.5, 0.3, 1.5)]
    starts = [sum(x0, ()), sum((tuple(v * 1.25 + 0.125 for v in x) for x in x0), ())]
    return makers, x0, starts


_memo = {}


def _batch_run(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _memo:
        makers, _, starts = _batch()
        objs = [m() for m in makers]
        _memo[key] = (HostRun(objs, starts, **kw), objs)
        assert _memo[key][0].rc == 0
    return _memo[key]


def test_trees_are_independent():
    """Each tree of a batch of twelve gets, bit for bit, the result it gets when it runs alone -- and the
    oracle's."""
    makers, x0, starts = _batch()
    assert sorted(m().n for m in makers) == [1] * 3 + [2] * 3 + [3] * 3 + [5] * 3
    host, _ = _batch_run()
    off = np.concatenate([[0], np.cumsum([m().n for m in makers])])
    for t, make in enumerate(makers):
        mine = [s[off[t]:off[t + 1]] for s in starts]
        alone = HostRun([make()], mine)
        assert alone.rc == 0 and host.result(t) == alone.result(0), t
        assert host.result(t) == oracle_best(make(), mine, 8), t
    # a tree without constants is skipped and its outputs are left alone
    with_empty = HostRun([None, makers[1](), None], [starts[0][1:3], starts[1][1:3]])
    assert with_empty.rc == 0 and with_empty.result(1) == host.result(1)
    assert with_empty.best_f[0] == -77.0 and with_empty.fcalls[2] == -77 and all(it[1] == 1 for it in with_empty.items)


SETTINGS = [dict(value_trials=vt, spec_slots=ss, spec_max_active=sa, spec_max_depth=sd)
            for vt in (0, 1) for ss in (0, 4, 32) for sa in (0, 64) for sd in (1, 64)]


def test_scheduling_is_invisible():
    """Value-only trials and speculation change which items a launch carries and nothing else."""
    base, _ = _batch_run(value_trials=0, spec_slots=0, spec_max_active=0, spec_max_depth=1)
    some_spec = 0
    for kw in SETTINGS:
        run, _ = _batch_run(**kw)
        assert run.results() == base.results(), kw
        spec = [it for it in run.items if it[4]]
        assert all(it[3] == kw["value_trials"] for it in spec), kw   # speculative items: value-only as the knob says
        if kw["spec_slots"] == 0 or kw["spec_max_active"] == 0:
            assert not spec, kw
        for call in range(run.ncalls):
            assert sum(1 for it in spec if it[0] == call) <= kw["spec_slots"], kw
        some_spec += len(spec)
        assert run.nlaunches == run.ncalls
    assert some_spec > 0
    # a failing line search costs fewer launches with speculation
    for name in ("exp_overflow", "log_wall", "quartic3_indefinite"):
        n0 = run_case(name, spec_slots=0)[0].nlaunches
        n32 = run_case(name, spec_slots=32)[0].nlaunches
        assert n32 < n0, (name, n32, n0)


@pytest.mark.parametrize("spec_slots", [0, 32])
def test_value_trials_ask_for_one_gradient_per_accepted_point(spec_slots):
    """With value-only trials, a tree's items with a gradient are its starts' first points, the Newton probes,
    each line search's first trial, and one re-evaluation of every point accepted later in a search: that
    point was given before, value-only, with the same objective bits, and it is the oracle's accepted point."""
    makers, x0, starts = _batch()
    run, objs = _batch_run(value_trials=1, spec_slots=spec_slots, spec_max_active=64, spec_max_depth=64)
    off = np.concatenate([[0], np.cumsum([m().n for m in makers])])
    for t, make in enumerate(makers):
        want_grad, later = 0, []
        for s in starts:
            oo = make()
            oracle_start(oo, s[off[t]:off[t + 1]], 8)
            p = parse_log(oo.log, oo.n)
            want_grad += 1 + len(p["probes"]) + len(p["searches"])
            for k, acc in enumerate(p["accepted"]):
                if p["searches"][k][0][0] != acc:  # accepted after the first trial
                    later.append((acc, p["searches"][k][-1][1]))
        mine = [it for it in run.items if it[1] == t]
        assert all(it[3] for it in mine if it[4])  # speculative: never a gradient
        with_grad = [it for it in mine if not it[3]]
        assert len(with_grad) == want_grad + len(later), t
        # the re-evaluations: gradient items at a point given value-only before
        redo = []
        for i, it in enumerate(mine):
            if not it[3] and any(p[3] and p[2] == it[2] for p in mine[:i]):
                prev = [p for p in mine[:i] if p[3] and p[2] == it[2]][-1]
                assert prev[5] == it[5]
                redo.append((it[2], it[5]))
        assert redo == later, t


def test_callback_error_ends_the_run():
    """A callback's status comes back as the call's result and the outputs stay untouched; bad arguments are
    refused."""
    for fail_at in (0, 3):
        run = HostRun([_rosen(2)], [(-1.2, 1.0)], fail_at=fail_at, fail_code=7)
        assert run.rc == 7 and run.ncalls == fail_at
        assert (run.best_x == -77.0).all() and (run.best_f == -77.0).all() and (run.fcalls == -77).all()
        assert run.nlaunches == -77
    lib = L.load()
    coff = np.array([0, 2], np.int64)
    st = np.array([-1.2, 1.0])
    out = np.zeros(2)
    fc = np.zeros(1, np.int64)
    cb = L.BFGS_EVAL_FN(lambda *a: 0)
    ok = dict(ntrees=1, nstarts=1, const_offsets=coff.ctypes.data, starts=st.ctypes.data, iterations=8, value_trials=1,
              spec_slots=32, spec_max_active=64, spec_max_depth=64)
    for bad in (dict(nstarts=0), dict(iterations=-1), dict(ntrees=-1), dict(spec_slots=-1), dict(const_offsets=None)):
        q = L.BfgsQuery(**{**ok, **bad})
        assert lib.srhip_bfgs_host(ctypes.byref(q), cb, None, L.ptr(out), L.ptr(out), L.ptr(fc), None) == L.ERR_INVALID, bad
    q = L.BfgsQuery(**ok)
    assert lib.srhip_bfgs_host(ctypes.byref(q), cb, None, None, L.ptr(out), L.ptr(fc), None) == L.ERR_INVALID
    assert lib.srhip_bfgs_host(None, cb, None, L.ptr(out), L.ptr(out), L.ptr(fc), None) == L.ERR_INVALID
