"""Every kernel instance spec_apply / spec_adjoint (hn_spectral.hip) dispatch to, against the float64 CPU oracle.  Needs a real MI355X.

Probes, reference and bar: tests/spectral_probes.py (noise, one Fourier mode per line along x and along y, impulses; float64 oracle; 1e-5 of
scale(n) * max|u|, scale(n) = max |L64(normalised noise)|).  tests/test_spectral_host.py shows on the CPU that an fp32 implementation meets this bar
with a factor 4 to spare and that a single wrong wavenumber entry fails it.  Every case prints its measured error as a fraction of that scale.

Routes ("Spectral routes and their tests"): radix-4 k_spec_cols / k_spec_rows<N> for the eight powers of two; the register-resident
256-point kernels (nine option combinations) and 512-point kernels (two routes); sixteen prime-factor instances k_spec_pfa<Q, P>, whose launch
shape (lines per block, dynamic LDS, the > 48 KB attribute path) depends on the batch; the dense operator.  Each with its adjoint twin where it
has one.

Measured on an MI355X, worst probe and size per route, error / (scale(n) * max|u|) against the bar of 1e-5 (the worst probe is a mode field
everywhere; the noise probe is 3 to 5 times smaller):
    radix-4, 16 ... 2048                       forward 7.6e-7   adjoint 8.5e-7   (both at 2048)
    256, spectral_radix16 0 / 1 / 2            4.6e-7 / 5.5e-7 / 5.5e-7; the three spectral_cols kernels give the same bits for each
    512, spectral_radix16 1 / 0                6.4e-7 / 5.7e-7
    prime-factor, all sixteen (Q, P)           forward 7.0e-7   adjoint 8.5e-7   (both at 1792, the > 48 KB launch)
    dense (and spectral_pfa 0)                 forward 6.3e-6   adjoint 5.7e-6   (both at 1040; <= 3.5e-6 up to 448)
    other PML widths, sigma_max, k             <= 1.7e-6 (dense 144), <= 5.9e-7 elsewhere
    rmse_hist against its residual slot        <= 1.5e-7 relative (bar 1e-5), every row kernel
    <L u, g> against <u, L^H g>                <= 2.1e-8 of |lhs| (bar 1e-5), every size
No case found a kernel wrong, and both header claims hold bit for bit.
"""
import ctypes

import pytest
import torch

import spectral_probes as SP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORWARD_SIZES = SP.forward_sizes()
ADJOINT_SIZES = SP.forward_sizes()
SRC_PER_SAMPLE_SIZES = [64, 256, 512, 320, 1792, 272]          # src_batch == batch (2): one size per kernel family
OPTIONS_256 = [(r, c) for r in (0, 1, 2) for c in (0, 1, 2)]   # (spectral_radix16, spectral_cols)
OPTIONS_512 = [0, 1]                                           # spectral_radix16
PFA_OFF_SIZES = [96, 320, 448]
BATCH_SHAPES = {768: (1, 2, 3), 1280: (1, 2), 1792: (1,)}
DOMAIN_CASES = ([(n, pml, SP.SIGMA_MAX, SP.K) for n in (48, 64, 144) for pml in (1, n // 2)]
                + [(n, SP.PML, s, k) for n in (96, 256) for s, k in ((0.5, 2.0), (0.0, 1.0))])
RMSE_CASES = [(64, 2, None), (256, 2, 0), (256, 2, 1), (256, 2, 2), (512, 1, 0), (512, 1, 1), (96, 2, None), (320, 1, None), (208, 1, None)]
DEFAULTS = {"spectral_radix16": 1, "spectral_cols": 1, "spectral_pfa": 1}


def pfa_launch_shape(n, batch):
    """(lines per block, dynamic LDS bytes) of launch_pfa (hn_spectral.hip) for a prime-factor size: what makes a batch a case of its own."""
    p, q = SP.pfa_factor(n)
    t = q // 4
    lpb = max(256 // t, 1)
    while lpb > 1 and lpb * 2 * p * q * 8 > 96 * 1024:
        lpb //= 2
    while lpb * t > 64 and ((n + lpb - 1) // lpb) * batch < 512:
        lpb //= 2
    return lpb, lpb * 2 * p * q * 8


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


def _fresh():
    from helmnet_amd.engine import Engine
    return Engine(DEV)


def _restore(e):
    try:
        for name, value in DEFAULTS.items():
            e.set_option(name, value)
    finally:
        e.close()


def _chunks(n, b):
    return [slice(s, s + 1) for s in range(b)] if n >= SP.ONE_AT_A_TIME else [slice(0, b)]


def _laplacian(e, n, u):
    """hn_laplacian through Engine.laplacian, and once more through the C entry into an output pre-filled with NaN: the row pass ADDS onto what
    the column pass left there, so a line either pass skipped shows as NaN (or as a difference).  -> the result on the CPU."""
    outs = []
    for sl in _chunks(n, u.shape[0]):
        x = u[sl].to(DEV)
        out = e.laplacian(x)
        again = torch.full_like(x, float("nan"))
        assert e.lib.hn_laplacian(e.ctx, _ptr(x), _ptr(again), x.shape[0], e._stream()) == 0
        assert not bool(torch.isnan(again).any()) and torch.equal(out, again)
        outs.append(out.cpu())
    return torch.cat(outs)


def _residual(e, n, u, k_sq, src):
    outs = []
    for sl in _chunks(n, u.shape[0]):
        x, kq = u[sl].to(DEV), k_sq[sl].to(DEV)
        s = (src if src.shape[0] == 1 else src[sl]).to(DEV)
        out = e.residual(x, kq, s)
        again = torch.full_like(x, float("nan"))
        assert e.lib.hn_residual(e.ctx, _ptr(x), _ptr(kq), _ptr(s), s.shape[0], _ptr(again), x.shape[0], e._stream()) == 0
        assert not bool(torch.isnan(again).any()) and torch.equal(out, again)
        outs.append(out.cpu())
    return torch.cat(outs)


def _vjp(e, n, g, k_sq):
    outs = []
    for sl in _chunks(n, g.shape[0]):
        x, kq = g[sl].to(DEV), k_sq[sl].to(DEV)
        out = e.residual_vjp(x, kq)
        again = torch.full_like(x, float("nan"))
        assert e.lib.hn_residual_vjp(e.ctx, _ptr(x), _ptr(kq), _ptr(again), x.shape[0], e._stream()) == 0
        assert not bool(torch.isnan(again).any()) and torch.equal(out, again)
        outs.append(out.cpu())
    return torch.cat(outs)


def _report(tag, what, got, want, bar, names=SP.PROBES):
    """Print error / bar * 1e-5 of every probe (the error as a fraction of the scale the bar is 1e-5 of) and return the worst ratio to the bar."""
    ratio = SP.errors(got, want) / bar[: got.shape[0]]
    print(f"SPEC {tag} {what}: " + ", ".join(f"{nm} {float(r) * SP.BAR:.2e}" for nm, r in zip(names, ratio)) + f"  (bar {SP.BAR:.0e})")
    return float(ratio.max())


def _check_forward(e, n, domain, tag):
    c = SP.forward_case(n, domain)
    lap = _laplacian(e, n, c["u"])
    res = _residual(e, n, c["u"], c["k_sq"], c["src1"])
    worst = max(_report(tag, "laplacian", lap, c["lap"], c["bar_lap"]), _report(tag, "residual", res, c["res1"], c["bar_res1"]))
    assert worst <= 1.0, (tag, worst * SP.BAR)
    return lap, res


def _check_adjoint(e, n, domain, tag):
    a = SP.adjoint_case(n, domain)
    vjp = _vjp(e, n, a["g"], a["k_sq"])
    worst = _report(tag, "adjoint", vjp, a["vjp"], a["bar"])
    assert worst <= 1.0, (tag, worst * SP.BAR)
    return vjp


# ------------------------------------------------------------------------------------------------------------------- 1: forward, every route
@pytest.mark.parametrize("n", FORWARD_SIZES)
def test_forward_matches_the_float64_oracle(eng, n):
    eng.set_domain(n, *SP.DOMAIN)
    _check_forward(eng, n, SP.DOMAIN, f"n={n} {SP.route(n)}")


@pytest.mark.parametrize("n", SRC_PER_SAMPLE_SIZES)
def test_residual_with_one_source_per_sample(eng, n):
    c = SP.forward_case(n)
    eng.set_domain(n, *SP.DOMAIN)
    x, kq, s = c["u"][:2].to(DEV), c["k_sq"][:2].to(DEV), c["src2"].to(DEV)
    out = eng.residual(x, kq, s)
    again = torch.full_like(x, float("nan"))
    assert eng.lib.hn_residual(eng.ctx, _ptr(x), _ptr(kq), _ptr(s), 2, _ptr(again), 2, eng._stream()) == 0
    assert torch.equal(out, again)
    assert _report(f"n={n} {SP.route(n)} src_batch=2", "residual", out, c["res2"], c["bar_res2"]) <= 1.0


@pytest.mark.parametrize("n,batch", [(48, 512), (80, 256)])
def test_prime_factor_blocks_with_dead_lines(eng, n, batch):
    """From 512 blocks on, a Q = 16 prime-factor launch keeps 64 lines per block: 48 lines leave 16 threads rows of the only block without a line, 80
    lines leave 48 of the second one.  Those threads take part in the barriers and must neither store nor count in the sum of squares."""
    assert pfa_launch_shape(n, batch)[0] == 64 and pfa_launch_shape(n, batch - 1)[0] < 64
    c = SP.forward_case(n)
    a = SP.adjoint_case(n)
    eng.set_domain(n, *SP.DOMAIN)
    few = eng.residual(c["u"].to(DEV), c["k_sq"].to(DEV), c["src1"].to(DEV))
    reps = batch // 4
    many = eng.residual(c["u"].repeat(reps, 1, 1, 1).to(DEV), c["k_sq"].repeat(reps, 1, 1, 1).to(DEV), c["src1"].to(DEV))
    assert _report(f"n={n} pfa batch={batch}", "residual", many[-4:], c["res1"], c["bar_res1"]) <= 1.0
    assert torch.equal(many.view(reps, 4, 2, n, n), few.expand(reps, 4, 2, n, n))
    g, kq = a["g"].to(DEV), a["k_sq"].to(DEV)
    reps = batch // 3 + 1
    many = eng.residual_vjp(g.repeat(reps, 1, 1, 1), kq.repeat(reps, 1, 1, 1))
    assert many.shape[0] >= batch and _report(f"n={n} pfa batch={many.shape[0]}", "adjoint", many[-3:], a["vjp"], a["bar"]) <= 1.0
    assert torch.equal(many.view(reps, 3, 2, n, n), eng.residual_vjp(g, kq).expand(reps, 3, 2, n, n))


# ------------------------------------------------------------------------------------------------------------------------------- 2: options
def test_all_nine_256_point_option_combinations():
    """spectral_radix16 x spectral_cols at 256: every combination against the oracle, and -- the header's claim for HN_OPT_SPECTRAL_COLS -- for a
    fixed spectral_radix16 in {1, 2} the three column kernels give the same bits (with 0 the option is not read: also the same bits)."""
    e = _fresh()
    try:
        e.set_domain(256, *SP.DOMAIN)
        out = {}
        for r, c in OPTIONS_256:
            e.set_option("spectral_radix16", r)
            e.set_option("spectral_cols", c)
            out[r, c] = _check_forward(e, 256, SP.DOMAIN, f"n=256 radix16={r} cols={c}")
        for r in (0, 1, 2):
            for c in (1, 2):
                assert torch.equal(out[r, c][0], out[r, 0][0]) and torch.equal(out[r, c][1], out[r, 0][1]), (r, c)
        # three different row kernels: the options do select something
        assert not torch.equal(out[0, 1][1], out[1, 1][1]) and not torch.equal(out[1, 1][1], out[2, 1][1])
    finally:
        _restore(e)


def test_both_512_point_routes():
    e = _fresh()
    try:
        e.set_domain(512, *SP.DOMAIN)
        out = {}
        for r in OPTIONS_512:
            e.set_option("spectral_radix16", r)
            out[r] = _check_forward(e, 512, SP.DOMAIN, f"n=512 radix16={r}")
        assert not torch.equal(out[0][1], out[1][1])
    finally:
        _restore(e)


@pytest.mark.parametrize("n", PFA_OFF_SIZES)
def test_dense_operator_on_prime_factor_sizes(n):
    """spectral_pfa = 0 is the dense operator (forward and adjoint tables) at a size the prime-factor kernels would take; setting it back to 1
    re-builds the tables and gives the bits of a context that never changed the option."""
    e, plain = _fresh(), _fresh()
    try:
        plain.set_domain(n, *SP.DOMAIN)
        want = _check_forward(plain, n, SP.DOMAIN, f"n={n} pfa")
        want_adj = _vjp(plain, n, SP.adjoint_case(n)["g"], SP.adjoint_case(n)["k_sq"])
        e.set_domain(n, *SP.DOMAIN)
        e.set_option("spectral_pfa", 0)
        dense = _check_forward(e, n, SP.DOMAIN, f"n={n} dense(spectral_pfa=0)")
        dense_adj = _check_adjoint(e, n, SP.DOMAIN, f"n={n} dense(spectral_pfa=0)")
        assert not torch.equal(dense[1], want[1]) and not torch.equal(dense_adj, want_adj)
        e.set_option("spectral_pfa", 1)
        back = _check_forward(e, n, SP.DOMAIN, f"n={n} pfa again")
        assert torch.equal(back[0], want[0]) and torch.equal(back[1], want[1])
        assert torch.equal(_vjp(e, n, SP.adjoint_case(n)["g"], SP.adjoint_case(n)["k_sq"]), want_adj)
    finally:
        _restore(e)
        plain.close()


# ------------------------------------------------------------------------------------------------------- 3: batch-dependent launch shapes
@pytest.mark.parametrize("n", sorted(BATCH_SHAPES))
def test_prime_factor_launch_shapes_by_batch(eng, n):
    """The lines per block (and with them the dynamic LDS: above 48 KB at 1792 and at 1280 from batch 2) follow the batch.  Each batch against the
    oracle, and sample 0 the same bits whatever shares its batch, forward and adjoint."""
    c, a = SP.forward_case(n), SP.adjoint_case(n)
    eng.set_domain(n, *SP.DOMAIN)
    first = None
    for b in BATCH_SHAPES[n]:
        lpb, lds = pfa_launch_shape(n, b)
        x, kq, s = c["u"][:b].to(DEV), c["k_sq"][:b].to(DEV), c["src1"].to(DEV)
        lap, res = eng.laplacian(x), eng.residual(x, kq, s)
        vjp = eng.residual_vjp(a["g"][:b].to(DEV), a["k_sq"][:b].to(DEV))
        tag = f"n={n} pfa batch={b} lines/block={lpb} lds={lds}"
        worst = max(_report(tag, "laplacian", lap, c["lap"][:b], c["bar_lap"]), _report(tag, "residual", res, c["res1"][:b], c["bar_res1"]),
                    _report(tag, "adjoint", vjp, a["vjp"][:b], a["bar"]))
        assert worst <= 1.0, (tag, worst * SP.BAR)
        if first is None:
            first = (lap, res, vjp)
        for one, many in zip(first, (lap, res, vjp)):
            assert torch.equal(one[0], many[0]), tag


@pytest.mark.parametrize("n", [256, 272])
def test_a_sample_does_not_depend_on_its_batch(eng, n):
    c, a = SP.forward_case(n), SP.adjoint_case(n)
    eng.set_domain(n, *SP.DOMAIN)
    x, kq, s = c["u"][:3].to(DEV), c["k_sq"][:3].to(DEV), c["src1"].to(DEV)
    g, gk = a["g"].to(DEV), a["k_sq"].to(DEV)
    lap, res, vjp = eng.laplacian(x), eng.residual(x, kq, s), eng.residual_vjp(g, gk)
    for i in range(3):
        assert torch.equal(eng.laplacian(x[i:i + 1])[0], lap[i])
        assert torch.equal(eng.residual(x[i:i + 1], kq[i:i + 1], s)[0], res[i])
        assert torch.equal(eng.residual_vjp(g[i:i + 1], gk[i:i + 1])[0], vjp[i])


# ------------------------------------------------------------------------------------------------------------------------------- 4: adjoint
@pytest.mark.parametrize("n", ADJOINT_SIZES)
def test_adjoint_matches_float64_autograd_and_the_forward_operator(eng, n):
    eng.set_domain(n, *SP.DOMAIN)
    vjp = _check_adjoint(eng, n, SP.DOMAIN, f"n={n} {SP.route(n)}")
    # <L u + k_sq u, g> == <u, L^H g + k_sq g> with the library's own forward operator, summed in float64: the bar of
    # test_training_gpu.test_residual_vjp_is_the_adjoint_of_the_residual
    # (u has a part along L^H g -- see adjoint_case -- so neither side is a sum that cancels and 1e-5 * |lhs| is a bar in units of the terms)
    a = SP.adjoint_case(n)
    u = a["u"]
    fwd = _residual(eng, n, u, a["k_sq"], torch.zeros(1, 2, n, n))
    lhs = (fwd.double() * a["g"].double()).flatten(1).sum(1)
    rhs = (u.double() * vjp.double()).flatten(1).sum(1)
    print(f"SPEC n={n} {SP.route(n)} identity: " + ", ".join(f"{nm} |lhs-rhs|/max(|lhs|,1) {abs(float(l - r)) / max(abs(float(l)), 1.0):.2e}"
                                                           for nm, l, r in zip(SP.PROBES, lhs, rhs)))
    for l, r in zip(lhs.tolist(), rhs.tolist()):
        assert abs(l - r) <= 1e-5 * max(abs(l), 1.0), (l, r)


# --------------------------------------------------------------------------------------------------------------------- 5: domain parameters
@pytest.mark.parametrize("n,pml,sigma_max,k", DOMAIN_CASES)
def test_other_domain_parameters(eng, n, pml, sigma_max, k):
    domain = (pml, sigma_max, k)
    eng.set_domain(n, *domain)
    tag = f"n={n} {SP.route(n)} pml={pml} sigma_max={sigma_max} k={k}"
    _check_forward(eng, n, domain, tag)
    _check_adjoint(eng, n, domain, tag)


def test_set_domain_still_refuses_a_pml_that_does_not_fit():
    e = _fresh()
    try:
        e.set_domain(48, *SP.DOMAIN)
        want = e.laplacian(SP.forward_case(48)["u"].to(DEV))
        for pml in (0, 25, -1):
            with pytest.raises(ValueError, match="does not fit"):
                e.set_domain(48, pml, SP.SIGMA_MAX, SP.K)
        assert e.lib.hn_set_domain(e.ctx, 48, 0, 2.0, 1.0) == -1 and e.lib.hn_set_domain(e.ctx, 48, 25, 2.0, 1.0) == -1
        e.set_domain(48, 24, SP.SIGMA_MAX, SP.K)                       # 2 * pml == n fits
        e.set_domain(48, *SP.DOMAIN)
        assert torch.equal(e.laplacian(SP.forward_case(48)["u"].to(DEV)), want)
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------- 6: fused RMSE per row kernel
@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    return s


@pytest.mark.parametrize("n,b,radix16", RMSE_CASES)
def test_fused_rmse_is_the_rmse_of_the_slot_it_belongs_to(solver, n, b, radix16):
    """hn_step sums the squares inside the row kernel into row *it_counter - 1 of the fp32 history.  Every row kernel: k_spec_rows (64; 256 and 512
    with spectral_radix16 0), k_spec8_rows, k_spec16_rows, k_spec512_rows, k_spec_pfa (96, 320), k_spec_dense (208)."""
    from helmnet_amd.phantoms import ring_sos_batch
    n_iter = 3
    solver.set_domain_size(n, source_location=[n // 8 + 4, n // 2])
    e = solver.engine()
    try:
        if radix16 is not None:
            e.set_option("spectral_radix16", radix16)
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
        e.set_option("spectral_radix16", DEFAULTS["spectral_radix16"])
    want = res_hist.double().pow(2).mean((2, 3, 4)).sqrt()
    got = guard[4:-4].double()
    assert bool(torch.isfinite(want).all()) and bool((want > 0).all())
    assert bool((guard[:4] == -7.0).all()) and bool((guard[-4:] == -7.0).all())       # exactly the n_iter rows were written
    rel = ((got - want).abs() / want)
    print(f"SPEC n={n} b={b} radix16={radix16} rmse_hist: max relative error {float(rel.max()):.2e}; rows {want[:, 0].tolist()}")
    assert float(rel.max()) <= 1e-5, rel.tolist()
    # rows that differ by more than the tolerance: a row filed under its neighbour would not pass
    assert float((want[1:] / want[:-1] - 1).abs().min()) > 1e-3
