"""The mixed spectral route (HN_OPT_SPECTRAL_MIXED 1: k_spec_line of hn_spectral_line.hip, n = P * 2^k with a runtime odd P) against the
float64 CPU oracle.  Needs a real MI355X.

Probes, reference and bar: tests/spectral_probes.py, unchanged (1e-5 of scale(n) * max|u|), plus the two extra mode fields of
tests/spectral_mixed_probes.py that carry the P / Q specific frequencies.  The checks are those of tests/test_spectral_gpu.py (a second call
through the C entry into a NaN-prefilled output, then torch.equal between the two calls); every case first asserts that the domain really runs
the mixed kernels (Engine.counter("spectral_route") == 4): a case that silently ran the dense operator would pass the bar too.

Sizes: the smallest at which each thing can go wrong -- spectral_mixed_probes.GPU_SIZES says why each is there.

Lines per block (rect_lines of hn_spectral_line.hip: 16 at most, 80 KB of line buffers at most, halved while ceil(n / lines) * batch < 512), by (n, batch):
    (144, 1) and (144, 3) -> 1,  (144, 33) -> 8,  (144, 64) -> 16,  (576, 1) -> 1,  (576, 5) -> 4       (test_a_sample_does_not_depend_on_its_batch)
    the forward cases (four probes per call): 144, 176, 240 -> 1;  288, 400, 1152 -> 2;  576 -> 4;  one sample per call: 1040 -> 2, 2032 -> 1.

Measured on an MI355X, worst probe, error / bar (the bar is 1e-5 of the scale; the restated fp32 algorithm of test_spectral_mixed_host.py gives
0.04 at 144 and 0.29 at 2032):
    n          144    176    240    288    400    576    1152   1040   2032
    forward    0.047  0.037  0.048  0.061  0.059  0.067  0.091  0.103  0.177
    adjoint    0.048  0.048  0.057  0.054  0.059  0.071  0.093  0.109  0.209
    <L u, g> against <u, L^H g>: <= 1.1e-8 of |lhs| (bar 1e-5);  rmse_hist against its residual slot: <= 3.1e-7 relative (bar 1e-5);
    one solver iteration against the oracle at 144 and 240: <= 7.8e-7 of max|want| (bar 1e-5).
"""
import ctypes

import pytest
import torch

import spectral_mixed_probes as MP
import spectral_probes as SP
import test_spectral_gpu as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = list(MP.GPU_SIZES)
SRC_PER_SAMPLE_SIZES = [144, 400]
ROUND_TRIP_SIZES = [144, 400]
BATCH_CASES = {144: (3, 33, 64), 576: (5,)}
RMSE_CASES = [(144, 2), (400, 1)]
STEP_SIZES = [144, 240]
DOMAIN_CASES = [(144, 1, SP.SIGMA_MAX, SP.K), (144, 72, SP.SIGMA_MAX, SP.K), (144, SP.PML, 0.5, 2.0)]
ROUTE_DENSE, ROUTE_PFA, ROUTE_MIXED = 3, 2, 4


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _fresh(mixed=1):
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    e.set_option("spectral_mixed", mixed)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _fresh()
    yield e
    e.close()


def _set_mixed_domain(e, n, domain=SP.DOMAIN):
    e.set_domain(n, *domain)
    assert e.counter("spectral_route") == ROUTE_MIXED, (n, e.counter("spectral_route"))


def _check_forward(e, n, domain, tag):
    """G._check_forward, and the same two calls on the two extra mode fields.  -> (laplacian, residual) of the four probes, the worst ratio."""
    c, x = SP.forward_case(n, domain), MP.extra_case(n, domain)
    lap, res = G._laplacian(e, n, c["u"]), G._residual(e, n, c["u"], c["k_sq"], c["src1"])
    lap2, res2 = G._laplacian(e, n, x["u"]), G._residual(e, n, x["u"], x["k_sq"], x["src1"])
    worst = max(G._report(tag, "laplacian", lap, c["lap"], c["bar_lap"]), G._report(tag, "residual", res, c["res1"], c["bar_res1"]),
                G._report(tag, "laplacian", lap2, x["lap"], x["bar_lap"], MP.EXTRA_NAMES),
                G._report(tag, "residual", res2, x["res1"], x["bar_res1"], MP.EXTRA_NAMES))
    print(f"MIXED {tag}: worst forward error / bar {worst:.3f}")
    assert worst <= 1.0, (tag, worst * SP.BAR)
    return lap, res


# ------------------------------------------------------------------------------------------------------------------------------- 1: forward
@pytest.mark.parametrize("n", SIZES)
def test_forward_matches_the_float64_oracle(eng, n):
    _set_mixed_domain(eng, n)
    p, q = MP.factor(n)
    _check_forward(eng, n, SP.DOMAIN, f"n={n} mixed {p}x{q}")


@pytest.mark.parametrize("n", SRC_PER_SAMPLE_SIZES)
def test_residual_with_one_source_per_sample(eng, n):
    c = SP.forward_case(n)
    _set_mixed_domain(eng, n)
    x, kq, s = c["u"][:2].to(DEV), c["k_sq"][:2].to(DEV), c["src2"].to(DEV)
    out = eng.residual(x, kq, s)
    again = torch.full_like(x, float("nan"))
    assert eng.lib.hn_residual(eng.ctx, _ptr(x), _ptr(kq), _ptr(s), 2, _ptr(again), 2, eng._stream()) == 0
    assert torch.equal(out, again)
    assert G._report(f"n={n} mixed src_batch=2", "residual", out, c["res2"], c["bar_res2"]) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------- 2: adjoint
@pytest.mark.parametrize("n", SIZES)
def test_adjoint_matches_float64_autograd_and_the_forward_operator(eng, n):
    _set_mixed_domain(eng, n)
    p, q = MP.factor(n)
    tag = f"n={n} mixed {p}x{q}"
    a = SP.adjoint_case(n)
    vjp = G._vjp(eng, n, a["g"], a["k_sq"])
    worst = G._report(tag, "adjoint", vjp, a["vjp"], a["bar"])
    print(f"MIXED {tag}: worst adjoint error / bar {worst:.3f}")
    assert worst <= 1.0, (tag, worst * SP.BAR)
    # <L u + k_sq u, g> == <u, L^H g + k_sq g> with the library's own forward operator, summed in float64: the identity and the tolerance of
    # test_spectral_gpu.test_adjoint_matches_float64_autograd_and_the_forward_operator
    u = a["u"]
    fwd = G._residual(eng, n, u, a["k_sq"], torch.zeros(1, 2, n, n))
    lhs = (fwd.double() * a["g"].double()).flatten(1).sum(1)
    rhs = (u.double() * vjp.double()).flatten(1).sum(1)
    print(f"MIXED {tag} identity: " + ", ".join(f"{nm} |lhs-rhs|/max(|lhs|,1) {abs(float(l - r)) / max(abs(float(l)), 1.0):.2e}"
                                                 for nm, l, r in zip(SP.PROBES, lhs, rhs)))
    for l, r in zip(lhs.tolist(), rhs.tolist()):
        assert abs(l - r) <= 1e-5 * max(abs(l), 1.0), (l, r)


# ------------------------------------------------------------------------------------------------------------------------- 3, 4: the option
@pytest.mark.parametrize("n", ROUND_TRIP_SIZES)
def test_option_round_trip_against_the_dense_operator(n):
    """0 is the dense operator, 1 the mixed kernels (other bits, same bar), back to 0 re-builds the dense tables: the first bits again."""
    e = _fresh(mixed=0)
    try:
        e.set_domain(n, *SP.DOMAIN)
        assert e.counter("spectral_route") == ROUTE_DENSE
        dense = G._check_forward(e, n, SP.DOMAIN, f"n={n} dense")
        dense_adj = G._check_adjoint(e, n, SP.DOMAIN, f"n={n} dense")
        e.set_option("spectral_mixed", 1)
        assert e.counter("spectral_route") == ROUTE_MIXED
        mixed = _check_forward(e, n, SP.DOMAIN, f"n={n} mixed after dense")
        mixed_adj = G._check_adjoint(e, n, SP.DOMAIN, f"n={n} mixed after dense")
        assert not torch.equal(mixed[0], dense[0]) and not torch.equal(mixed[1], dense[1]) and not torch.equal(mixed_adj, dense_adj)
        e.set_option("spectral_mixed", 0)
        assert e.counter("spectral_route") == ROUTE_DENSE
        back = G._check_forward(e, n, SP.DOMAIN, f"n={n} dense again")
        assert torch.equal(back[0], dense[0]) and torch.equal(back[1], dense[1])
        assert torch.equal(G._vjp(e, n, SP.adjoint_case(n)["g"], SP.adjoint_case(n)["k_sq"]), dense_adj)
    finally:
        e.close()


def test_prime_factor_size_on_the_mixed_kernels():
    """96 = 3 * 32 belongs to the prime-factor kernels; with spectral_pfa 0 and spectral_mixed 1 the mixed ones take it (P = 3 is an odd factor
    like any other).  Restoring both options gives the prime-factor bits back."""
    n = 96
    e = _fresh(mixed=0)
    try:
        assert e.counter("spectral_route") == 0                      # no domain yet
        e.set_domain(n, *SP.DOMAIN)
        assert e.counter("spectral_route") == ROUTE_PFA
        want = G._check_forward(e, n, SP.DOMAIN, f"n={n} pfa")
        want_adj = G._check_adjoint(e, n, SP.DOMAIN, f"n={n} pfa")
        e.set_option("spectral_mixed", 1)
        assert e.counter("spectral_route") == ROUTE_PFA              # the prime-factor kernels keep their sizes
        e.set_option("spectral_pfa", 0)
        assert e.counter("spectral_route") == ROUTE_MIXED
        mixed = _check_forward(e, n, SP.DOMAIN, f"n={n} mixed 3x32 (spectral_pfa=0)")
        mixed_adj = G._check_adjoint(e, n, SP.DOMAIN, f"n={n} mixed 3x32 (spectral_pfa=0)")
        assert not torch.equal(mixed[1], want[1]) and not torch.equal(mixed_adj, want_adj)
        e.set_option("spectral_pfa", 1)
        e.set_option("spectral_mixed", 0)
        assert e.counter("spectral_route") == ROUTE_PFA
        back = G._check_forward(e, n, SP.DOMAIN, f"n={n} pfa again")
        assert torch.equal(back[0], want[0]) and torch.equal(back[1], want[1])
        assert torch.equal(G._vjp(e, n, SP.adjoint_case(n)["g"], SP.adjoint_case(n)["k_sq"]), want_adj)
        e.set_domain(256, *SP.DOMAIN)
        assert e.counter("spectral_route") == 1
        with pytest.raises(ValueError, match="HN_OPT_SPECTRAL_MIXED"):
            e.set_option("spectral_mixed", 2)
    finally:
        e.close()


def test_environment_default_goes_through_the_option_validator(monkeypatch):
    """HN_SPECTRAL_MIXED is read once, in hn_create, as the default of the option: 1 routes 144 to the mixed kernels, a value hn_set_option
    would reject fails the creation."""
    from helmnet_amd.engine import Engine
    monkeypatch.setenv("HN_SPECTRAL_MIXED", "1")
    e = Engine(DEV)
    try:
        e.set_domain(144, *SP.DOMAIN)
        assert e.counter("spectral_route") == ROUTE_MIXED
    finally:
        e.close()
    monkeypatch.setenv("HN_SPECTRAL_MIXED", "2")
    with pytest.raises(ValueError, match="HN_SPECTRAL_MIXED"):
        Engine(DEV)
    monkeypatch.delenv("HN_SPECTRAL_MIXED")
    e = Engine(DEV)
    try:
        e.set_domain(144, *SP.DOMAIN)
        assert e.counter("spectral_route") == ROUTE_DENSE          # the default is off
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------- 5: batch independence
@pytest.mark.parametrize("n", sorted(BATCH_CASES))
def test_a_sample_does_not_depend_on_its_batch(eng, n):
    """Batch 1 against the batches of BATCH_CASES: every lines-per-block choice of rect_lines (module docstring), forward and adjoint."""
    c, x, a = SP.forward_case(n), MP.extra_case(n), SP.adjoint_case(n)
    _set_mixed_domain(eng, n)
    assert len({MP.mixed_lines(n, 4, b) for b in (1,) + BATCH_CASES[n]}) > 1 and len({MP.mixed_lines(n, 3, b) for b in (1,) + BATCH_CASES[n]}) > 1
    u = torch.cat([c["u"], x["u"]]).to(DEV)
    kq = torch.cat([c["k_sq"], x["k_sq"]]).to(DEV)
    s = c["src1"].to(DEV)
    d = u.shape[0]
    one = [(eng.laplacian(u[i:i + 1])[0], eng.residual(u[i:i + 1], kq[i:i + 1], s)[0], eng.residual_vjp(u[i:i + 1], kq[i:i + 1])[0]) for i in range(d)]
    for b in BATCH_CASES[n]:
        idx = [j % d for j in range(b)]
        ub, kb = u[idx].contiguous(), kq[idx].contiguous()
        many = (eng.laplacian(ub), eng.residual(ub, kb, s), eng.residual_vjp(ub, kb))
        for j, i in enumerate(idx):
            for got, want in zip(many, one[i]):
                assert torch.equal(got[j], want), (n, b, j)


# ----------------------------------------------------------------------------------------------------------------------- 6, 7: the solver
@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    return s


@pytest.mark.parametrize("n,b", RMSE_CASES)
def test_fused_rmse_is_the_rmse_of_the_slot_it_belongs_to(solver, n, b):
    """The body of test_spectral_gpu's test of the same name on the mixed row pass: three hn_step iterations, sentinel rows around the history."""
    from helmnet_amd.phantoms import ring_sos_batch
    n_iter = 3
    solver.set_domain_size(n, source_location=[n // 8 + 4, n // 2])
    e = solver.engine()
    try:
        e.set_option("spectral_mixed", 1)
        assert e.counter("spectral_route") == ROUTE_MIXED
        k_sq = ((1.0 / torch.from_numpy(ring_sos_batch(n, b, seed=21 + n))) ** 2).float().to(DEV).contiguous()
        src = solver._src()
        wf = torch.zeros(b, 2, n, n, device=DEV)
        res = e.residual(wf, k_sq, src)
        states = torch.zeros(b, 2, e.state_len, device=DEV)
        res_hist = torch.full((n_iter, b, 2, n, n), float("nan"), device=DEV)
        guard = torch.full((n_iter + 8, b), -7.0, device=DEV)        # four sentinel rows each side (the table stays 16-byte aligned)
        e.step(wf, res, states, k_sq, src, n_iter, res_hist=res_hist, rmse_hist=guard[4:-4])
        torch.cuda.synchronize()
        e.check_async_errors()
    finally:
        e.set_option("spectral_mixed", 0)
    want = res_hist.double().pow(2).mean((2, 3, 4)).sqrt()
    got = guard[4:-4].double()
    assert bool(torch.isfinite(want).all()) and bool((want > 0).all())
    assert bool((guard[:4] == -7.0).all()) and bool((guard[-4:] == -7.0).all())       # exactly the n_iter rows were written
    rel = ((got - want).abs() / want)
    print(f"MIXED n={n} b={b} rmse_hist: max relative error {float(rel.max()):.2e}; rows {want[:, 0].tolist()}")
    assert float(rel.max()) <= 1e-5, rel.tolist()
    assert float((want[1:] / want[:-1] - 1).abs().min()) > 1e-3


@pytest.mark.parametrize("n", STEP_SIZES)
def test_single_step_against_the_oracle(solver, n, weights):
    """One solver iteration with the shipped weights on the mixed route: the inputs and the bar (1e-5 of max|want|) of
    test_gpu_parity.test_ops_vs_oracle_other_sizes."""
    from golden_inputs import teacher_inputs
    from oracle import helmnet_oracle as O
    ti = {k: torch.from_numpy(v) for k, v in teacher_inputs(n, 1, seed=77 + n).items()}
    loc = [n // 4, n // 2]
    solver.set_domain_size(n, source_location=loc)
    t = O.SpectralTables(n, 8, 2, 1.0)
    src = O.point_source_map(n, loc, 10.0)
    k_sq_o, _ = O.get_initials(ti["sos"], 1.0)
    st = O.unflatten_states(ti["states"], n, 4)
    want_wf, want_res, want_st = O.single_step(ti["wf"], k_sq_o, ti["res"], st, weights, src, t)
    want_lap = O.apply_laplacian(ti["wf"], t)
    e = solver.engine()
    try:
        e.set_option("spectral_mixed", 1)
        assert e.counter("spectral_route") == ROUTE_MIXED
        g = {k: v.to(DEV) for k, v in ti.items()}
        k_sq, _ = solver.get_initials(g["sos"])
        lap = solver.apply_laplacian(g["wf"]).cpu()
        solver.f.set_states(g["states"], flatten=True)
        wf2, res2 = solver.single_step(g["wf"], k_sq, g["res"])
        st2 = solver.f.get_states(flatten=True).cpu()
        assert e.counter("spectral_route") == ROUTE_MIXED
    finally:
        e.set_option("spectral_mixed", 0)
    errs = {
        "lap": ((lap - want_lap).abs().max() / want_lap.abs().max()).item(),
        "wf": ((wf2.cpu() - want_wf).abs().max() / want_wf.abs().max()).item(),
        "res": ((res2.cpu() - want_res).abs().max() / want_res.abs().max()).item(),
        "st": ((st2 - O.flatten_states(want_st)).abs().max() / O.flatten_states(want_st).abs().max()).item(),
    }
    print(f"MIXED n={n} single_step against the oracle: {errs}")
    assert all(v <= 1e-5 for v in errs.values()), errs


# --------------------------------------------------------------------------------------------------------------------- 8: domain parameters
@pytest.mark.parametrize("n,pml,sigma_max,k", DOMAIN_CASES)
def test_other_domain_parameters(eng, n, pml, sigma_max, k):
    domain = (pml, sigma_max, k)
    _set_mixed_domain(eng, n, domain)
    tag = f"n={n} mixed pml={pml} sigma_max={sigma_max} k={k}"
    _check_forward(eng, n, domain, tag)
    G._check_adjoint(eng, n, domain, tag)


# ------------------------------------------------------------------------------------------------------------------------ 9: stream capture
def test_first_call_after_set_domain_can_be_captured():
    """hn_set_domain sets the kernels' dynamic-LDS attribute, so the first residual on a new domain is nothing but launches: it is captured, and
    one replay gives the bits of the eager call."""
    n = 144
    c = SP.forward_case(n)
    e = _fresh()
    try:
        _set_mixed_domain(e, n)
        x, kq, s = c["u"].to(DEV), c["k_sq"].to(DEV), c["src1"].to(DEV)
        out = torch.full_like(x, float("nan"))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = e.lib.hn_residual(e.ctx, _ptr(x), _ptr(kq), _ptr(s), 1, _ptr(out), x.shape[0], e._stream())
            assert rc == 0, e.lib.hn_last_error(e.ctx)
            out.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
        eager = e.residual(x, kq, s)
        assert not bool(torch.isnan(out).any()) and torch.equal(out, eager)
        assert G._report(f"n={n} mixed captured", "residual", out, c["res1"], c["bar_res1"]) <= 1.0
    finally:
        e.close()
