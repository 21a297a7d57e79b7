"""hn_residual_f64_lossy on the GPU: the float64 residual of an absorbing medium, L(u) + (k_sq + i k_sq_im) u - src, on square and rectangular
domains, and ``IterativeSolver.verify(absorption=...)``.  Needs a real MI355X.

Expected values come from tests/lossy_common.py (``LC.forward_case`` / ``LC.residual``: the oracle's Laplacian on the per-axis float64 tables of
tests/rect_common.py plus the complex term), from ``LA.lossy_matrix`` (the oracle's explicit-matrix assembly) and from the per-axis matrices
M_H U + U M_W^T; tests/test_f64_lossy_host.py pins the first against the last to 1e-12.  None of it comes from the code under test.

Bars, those of test_f64_gpu.py / test_f64_fft_gpu.py (derived there): against the float64 reference max abs error <= 1e-11 * max|expected|; one
evaluation against another 2e-11 (triangle inequality); rmse against the returned field 1e-14 relative.  ``evaluator_error`` of verify(): the bar
tests/test_lossy_gpu.py holds hn_residual_lossy to, SP.BAR * (scale * max|u| + max(|k~^2| |u|) + max|src|) -- an RMSE is at most the max error."""
import ctypes

import numpy as np
import pytest
import torch

import lossy_adjoint_common as LA
import lossy_common as LC
import rect_common as R
import spectral_probes as SP
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-11
OK, ERR_ARG, ERR_STATE = 0, -1, -2
# P = 1 (even and odd log2 Q), 3, 5, 9, 17 (Q = 16), and the headline size
SQUARES = (16, 32, 48, 80, 144, 272)
# P = 1 against 5; 5 against 3; both passes on the smallest lines; 16 lines per block in the column pass against 1 in the row pass (batch 4); the
# longest four-buffer line in the column pass
RECTANGLES = ((32, 80), (80, 48), (48, 16), (16, 2048), (2032, 16))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _err(e):
    return e.lib.hn_last_error(e.ctx).decode()


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


def _rel(got, want):
    return float((got.cpu() - want).abs().max()) / float(want.abs().max())


def _dev64(c, src="srcb", samples=None):
    sl = slice(None) if samples is None else slice(0, samples)
    s = c[src] if c[src].shape[0] == 1 else c[src][sl]
    return tuple(t.double().contiguous().to(DEV) for t in (c["u"][sl], c["k_sq"][sl], c["k_sq_im"][sl], s))


_big = {}


def _one_sample_case(n):
    """One sample at a large n x n (the four probes of LC.forward_case would cost gigabytes of float64 on the host): the noise probe, seeded media and
    source, and ``LC.residual`` on the float64 tables."""
    if n not in _big:
        u = R.noise_field(n, n)[None].contiguous()
        k_sq, k_im, src = R.seeded_k_sq(n, n, 1, 5000 + 4 * n), LC.seeded_k_sq_im(n, n, 1, 8000 + 4 * n, flip=0).abs(), R.seeded_src(n, n, 1, 6000 + 4 * n)
        want = LC.residual(u.double(), k_sq.double(), k_im.double(), src.double(), R.tables(n, n)).contiguous()
        _big[n] = dict(u=u, k_sq=k_sq, k_sq_im=k_im, srcb=src, lresb=want)
    return _big[n]


# ------------------------------------------------------------------------------------------------------------------ 1, 2: the float64 reference
@pytest.mark.parametrize("n", SQUARES)
def test_squares_match_the_float64_reference(eng, n):
    c = LC.forward_case(n, n)
    eng.set_domain(n, *R.DOMAIN)
    for src, name in (("srcb", "lresb"), ("src1", "lres1")) if n == 48 else (("srcb", "lresb"),):
        res, rmse = eng.residual64_lossy(*_dev64(c, src))
        assert eng.counter("f64_route") == 2 and res.dtype == rmse.dtype == torch.float64
        e = _rel(res, c[name])
        print(f"F64 LOSSY {n}x{n} (P, Q) {R.factor(n)} src batch {c[src].shape[0]}: {e:.3e} of max|expected|")
        assert e <= BAR, e


def test_two_samples_at_256(eng):
    c = LC.forward_case(256, 256)
    eng.set_domain(256, *R.DOMAIN)
    res, _ = eng.residual64_lossy(*_dev64(c, samples=2))
    e = _rel(res, c["lresb"][:2])
    print(f"F64 LOSSY 256x256 x 2: {e:.3e} of max|expected|")
    assert e <= BAR, e


@pytest.mark.parametrize("n", [2032, 2048])
def test_one_sample_at_the_longest_lines(eng, n):
    c = _one_sample_case(n)
    eng.set_domain(n, *R.DOMAIN)
    res, _ = eng.residual64_lossy(*_dev64(c))
    e = _rel(res, c["lresb"])
    print(f"F64 LOSSY {n}x{n} (P, Q) {R.factor(n)}: {e:.3e} of max|expected|")
    assert e <= BAR, e


@pytest.mark.parametrize("h,w", RECTANGLES)
def test_rectangles_match_the_float64_reference(eng, h, w):
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    worst = {}
    for src, name in (("srcb", "lresb"), ("src1", "lres1")):
        res, rmse = eng.residual64_lossy(*_dev64(c, src))
        assert eng.counter("f64_route") == 2 and tuple(res.shape) == (4, 2, h, w)
        worst[name] = _rel(res, c[name])
        want = c[name].pow(2).mean((1, 2, 3)).sqrt()
        assert float(((rmse.cpu() - want).abs() / want).max()) <= BAR
    print(f"F64 LOSSY {h}x{w} (P, Q) rows {R.factor(w)} columns {R.factor(h)}: {worst} of max|expected|")
    assert max(worst.values()) <= BAR, worst


# ------------------------------------------------------------------------------------------------------------------ 3: assembled operators
@pytest.mark.parametrize("n", [16, 48])
def test_squares_match_the_assembled_lossy_matrix(eng, n):
    c = LC.forward_case(n, n)
    eng.set_domain(n, *R.DOMAIN)
    res, _ = eng.residual64_lossy(*_dev64(c))
    for i in range(c["u"].shape[0]):
        mat = LA.lossy_matrix(c["k_sq"][i, 0].numpy(), c["k_sq_im"][i, 0].numpy())
        u = (c["u"][i, 0].double().numpy() + 1j * c["u"][i, 1].double().numpy()).reshape(-1)
        s = (c["srcb"][i, 0].double().numpy() + 1j * c["srcb"][i, 1].double().numpy()).reshape(-1)
        want = (mat @ u - s).reshape(n, n)
        got = res[i].cpu().numpy()
        err = max(np.abs(got[0] - want.real).max(), np.abs(got[1] - want.imag).max())
        assert err <= BAR * np.abs(want).max(), (i, err, np.abs(want).max())


def test_a_rectangle_matches_the_per_axis_matrices(eng):
    h, w = 32, 80
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    res, _ = eng.residual64_lossy(*_dev64(c))
    mh, mw = O.axis_operator_matrix(h, *R.DOMAIN), O.axis_operator_matrix(w, *R.DOMAIN)
    for i in range(c["u"].shape[0]):
        u = c["u"][i, 0].double().numpy() + 1j * c["u"][i, 1].double().numpy()
        kk = c["k_sq"][i, 0].double().numpy() + 1j * c["k_sq_im"][i, 0].double().numpy()
        s = c["srcb"][i, 0].double().numpy() + 1j * c["srcb"][i, 1].double().numpy()
        want = mh @ u + u @ mw.T + kk * u - s
        got = res[i].cpu().numpy()
        err = np.abs((got[0] + 1j * got[1]) - want).max()
        assert err <= BAR * np.abs(want).max(), (i, err)


# ------------------------------------------------------------------------------------------------------------------ 4: zero absorption
@pytest.mark.parametrize("n,b", [(16, 4), (48, 4), (256, 2)])
def test_zero_absorption_is_the_lossless_fft_route_bit_for_bit(eng, n, b):
    c = LC.forward_case(n, n)
    u, k_sq, _, src = _dev64(c, samples=b)
    zero = torch.zeros_like(k_sq)
    eng.set_domain(n, *R.DOMAIN)
    eng.set_option("f64_fft", 0)
    try:
        dense_res, dense_rmse = eng.residual64(u, k_sq, src)
        assert eng.counter("f64_route") == 1
        lossy_res, lossy_rmse = eng.residual64_lossy(u, k_sq, zero, src)          # the option does not reach the lossy call
        assert eng.counter("f64_route") == 2
        again_res, again_rmse = eng.residual64(u, k_sq, src)
        assert eng.counter("f64_route") == 1
        assert torch.equal(again_res, dense_res) and torch.equal(again_rmse, dense_rmse)      # the dense tables and bits, untouched
        eng.set_option("f64_fft", 1)
        fft_res, fft_rmse = eng.residual64(u, k_sq, src)
        assert eng.counter("f64_route") == 2
        assert torch.equal(lossy_res, fft_res) and torch.equal(lossy_rmse, fft_rmse)
        res2, rmse2 = eng.residual64_lossy(u, k_sq, zero, src)
        assert torch.equal(res2, fft_res) and torch.equal(rmse2, fft_rmse)
        assert torch.equal(eng.residual64_lossy(u, k_sq, zero, src, want_res=False)[1], eng.residual64(u, k_sq, src, want_res=False)[1])
    finally:
        eng.set_option("f64_fft", 0)


# ------------------------------------------------------------------------------------------------------------------ 5: rmse
@pytest.mark.parametrize("h,w", [(48, 48), (32, 80), (16, 2048)])
def test_rmse_is_the_rmse_of_the_returned_field_and_reproducible(eng, h, w):
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    args = _dev64(c)
    res, rmse = eng.residual64_lossy(*args)
    want = res.pow(2).mean((1, 2, 3)).sqrt()
    assert rmse.dtype == torch.float64 and rmse.shape == (4,)
    assert float(((rmse - want).abs() / want).max()) <= 1e-14
    res2, rmse2 = eng.residual64_lossy(*args)
    assert torch.equal(rmse, rmse2) and torch.equal(res, res2)
    only_rmse = eng.residual64_lossy(*args, want_res=False)            # res == NULL: the column pass writes the library's [B,2,h,w] field
    only_res = eng.residual64_lossy(*args, want_rmse=False)
    assert only_rmse[0] is None and torch.equal(only_rmse[1], rmse)
    assert only_res[1] is None and torch.equal(only_res[0], res)


# (256, 256) x 8: four lines per block where the sample alone runs one; (16, 2048) x 4: 16 lines per block in the column pass where the sample alone runs 4
@pytest.mark.parametrize("h,w,batch", [(256, 256, 8), (16, 2048, 4)])
def test_a_samples_bits_do_not_depend_on_its_batch(eng, h, w, batch):
    g = torch.Generator().manual_seed(4100 + h + w + batch)
    wf = torch.randn(batch, 2, h, w, generator=g, dtype=torch.float32).double().to(DEV)
    k_sq = (1.0 / (1.0 + torch.rand(batch, 1, h, w, generator=g, dtype=torch.float32)) ** 2).double().to(DEV)
    k_im = (0.3 * torch.rand(batch, 1, h, w, generator=g, dtype=torch.float32)).double().to(DEV)
    src = torch.randn(batch, 2, h, w, generator=g, dtype=torch.float32).double().to(DEV)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    res, rmse = eng.residual64_lossy(wf, k_sq, k_im, src)
    rmse_only = eng.residual64_lossy(wf, k_sq, k_im, src, want_res=False)[1]
    for i in (0, batch - 1):
        one = [t[i:i + 1].contiguous() for t in (wf, k_sq, k_im, src)]
        res1, rmse1 = eng.residual64_lossy(*one)
        assert torch.equal(res1[0], res[i]) and torch.equal(rmse1[0], rmse[i]) and torch.equal(rmse_only[i], rmse[i])


# ------------------------------------------------------------------------------------------------------------------ 6: transposition
@pytest.mark.parametrize("h,w", [(32, 80), (48, 16)])
def test_the_transposed_problem_gives_the_transposed_residual(eng, h, w):
    c = LC.forward_case(h, w)
    args = _dev64(c)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    res, rmse = eng.residual64_lossy(*args)
    eng.set_domain_rect(w, h, *R.DOMAIN)
    res_t, rmse_t = eng.residual64_lossy(*(t.transpose(-1, -2).contiguous() for t in args))
    d = float((res_t.transpose(-1, -2) - res).abs().max()) / float(res.abs().max())
    d_rmse = float(((rmse_t - rmse).abs() / rmse).max())
    print(f"F64 LOSSY {h}x{w} against {w}x{h} on transposed inputs: {d:.3e} of max, rmse {d_rmse:.3e} relative")
    assert d <= 2 * BAR and d_rmse <= 2 * BAR


# ------------------------------------------------------------------------------------------------------------------ 7, 8: caller buffers
def _off_by_one_double(t):
    """The same values in a tensor that starts one double into a larger allocation (8-byte aligned, no more)."""
    big = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = big[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 8
    return view


@pytest.mark.parametrize("h,w", [(48, 48), (32, 80)])
def test_eight_byte_aligned_tensors_give_the_aligned_bits(eng, h, w):
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    args = _dev64(c)
    want_res, want_rmse = eng.residual64_lossy(*args)
    u, k_sq, k_im, src = (_off_by_one_double(t) for t in args)
    out, rmse = _off_by_one_double(torch.zeros_like(want_res)), _off_by_one_double(torch.zeros_like(want_rmse))
    assert eng.lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), _ptr(k_im), _ptr(src), 4, _ptr(out), _ptr(rmse), 4, eng._stream()) == OK
    assert torch.equal(out, want_res) and torch.equal(rmse, want_rmse)


def test_refusals_write_nothing(eng):
    h, w, b = 32, 80, 4
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    u, k_sq, k_im, src = _dev64(c)
    lib, stream = eng.lib, eng._stream()
    out, rmse = torch.full_like(u, 7.0), torch.full((b,), 7.0, device=DEV, dtype=torch.float64)
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), None, _ptr(src), b, _ptr(out), _ptr(rmse), b, stream) == ERR_ARG
    assert "hn_residual_f64" in _err(eng).replace("hn_residual_f64_lossy", "") and "k_sq_im" in _err(eng)      # names the lossless sibling
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), _ptr(k_im), _ptr(src), b, None, None, b, stream) == ERR_ARG
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), _ptr(k_im), _ptr(src), 2, _ptr(out), _ptr(rmse), b, stream) == ERR_ARG
    # wf overlapping res, k_sq_im overlapping res: refused with nothing written
    both = torch.zeros(2 * u.numel(), device=DEV, dtype=torch.float64)
    both[: u.numel()].copy_(u.reshape(-1))
    before = both.clone()
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(both), _ptr(k_sq), _ptr(k_im), _ptr(src), b, _ptr(both[u.numel() // 2:]), _ptr(rmse), b, stream) == ERR_ARG
    assert "wf" in _err(eng)
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(both), _ptr(k_sq), _ptr(k_im), _ptr(src), b, _ptr(both), None, b, stream) == ERR_ARG
    kbuf = torch.zeros(u.numel() + k_im.numel(), device=DEV, dtype=torch.float64)
    kbuf[u.numel():].copy_(k_im.reshape(-1))
    kbefore = kbuf.clone()
    assert lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), _ptr(kbuf[u.numel() - 8:]), _ptr(src), b, _ptr(kbuf), _ptr(rmse), b, stream) == ERR_ARG
    assert "k_sq_im" in _err(eng)
    torch.cuda.synchronize()
    assert torch.equal(both, before) and torch.equal(kbuf, kbefore) and bool((out == 7.0).all()) and bool((rmse == 7.0).all())
    res, _ = eng.residual64_lossy(u, k_sq, k_im, src)                      # and the context still works
    assert _rel(res, c["lresb"]) <= BAR


# ------------------------------------------------------------------------------------------------------------------ 9: capture
@pytest.mark.parametrize("h,w", [(48, 48), (32, 80)])
def test_first_call_refuses_capture_and_later_calls_are_capturable(eng, h, w):
    c = LC.forward_case(h, w)
    u, k_sq, k_im, src = _dev64(c)
    b = u.shape[0]
    out, rmse = torch.full_like(u, 7.0), torch.empty(b, device=DEV, dtype=torch.float64)
    eng.set_domain(16, *R.DOMAIN)
    eng.set_domain_rect(h, w, *R.DOMAIN)                                 # a fresh domain: no float64 tables yet
    call = lambda o, r: eng.lib.hn_residual_f64_lossy(eng.ctx, _ptr(u), _ptr(k_sq), _ptr(k_im), _ptr(src), b, _ptr(o), _ptr(r), b, eng._stream())  # noqa: E731
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rmse.zero_()
            rc = call(out, rmse)
        assert rc == ERR_STATE                                         # would have to build the tables: refused before anything is enqueued
        graph.replay()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                                # the refused call left out untouched
        assert eng.counter("f64_route") == 0
        want_res, want_rmse = eng.residual64_lossy(u, k_sq, k_im, src)     # eager: builds them
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc_none = call(None, rmse)
        assert rc_none == ERR_STATE                                    # rmse only: the intermediate field does not exist yet
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call(out, rmse)
        assert rc == OK
        out.zero_()
        rmse.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, want_res) and torch.equal(rmse, want_rmse)


# ------------------------------------------------------------------------------------------------------------------ 10: verify(absorption=...)
@pytest.mark.parametrize("size,loc", [(64, [20, 32]), ((32, 80), [8, 40])])
def test_verify_with_absorption(size, loc):
    from helmnet_amd import IterativeSolver
    from helmnet_amd.absorption import complex_k_sq
    h, w = (size, size) if isinstance(size, int) else size
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    s.set_domain_size(size, source_location=loc)
    eng = s.engine()
    c = LC.forward_case(h, w)
    wf = c["u"].to(DEV)
    g = torch.Generator().manual_seed(64 + h + w)
    sos = (1.0 + torch.rand(4, 1, h, w, generator=g, dtype=torch.float32)).to(DEV)
    alpha = (0.1 * (sos - 1.0)).contiguous()
    k_sq, k_im = complex_k_sq(sos, alpha, s.hparams.omega)              # the fp32 planes the solver forms (pinned by tests/test_lossy_host.py)
    src = s.source.detach().float().contiguous()
    out = s.verify(wf, sos_maps=sos, absorption=alpha)
    assert sorted(out) == ["evaluator_error", "residual_norm32", "residual_norm64"]
    res64, norm64 = eng.residual64_lossy(wf.double(), k_sq.double(), k_im.double(), src.double())
    res32 = eng.residual_lossy(wf, k_sq.contiguous(), k_im.contiguous(), src)
    assert torch.equal(out["residual_norm64"], norm64)
    norm32 = res32.double().pow(2).mean((1, 2, 3)).sqrt()
    assert float(((out["residual_norm32"].double() - norm32).abs() / norm32).max()) <= 1e-5      # hn_rmse: fp32, one atomicAdd per block
    want = (res32.double() - res64).pow(2).mean((1, 2, 3)).sqrt()
    assert float(((out["evaluator_error"] - want).abs() / want).max()) <= 1e-14
    # the other pairing, and the keyword of get_residual64: the same bits
    out2 = s.verify(wf, k_sq=k_sq, k_sq_im=k_im)
    assert torch.equal(out["residual_norm64"], out2["residual_norm64"]) and torch.equal(out["evaluator_error"], out2["evaluator_error"])
    assert torch.equal(s.get_residual64(wf, k_sq, k_sq_im=k_im), res64)
    # the float64 residual is the reference's (the source is the solver's own map)
    ref = LC.residual(wf.cpu().double(), k_sq.cpu().double(), k_im.cpu().double(), src.cpu().double(), R.tables(h, w))
    assert _rel(res64, ref) <= BAR
    mag = torch.sqrt(k_sq.cpu().double() ** 2 + k_im.cpu().double() ** 2) * wf.cpu().double().abs()
    bar = SP.BAR * (c["scale"] * SP.peak(wf.cpu()) + SP.peak(mag) + float(src.abs().max()))
    ratio = out["evaluator_error"].cpu() / bar
    print(f"verify(absorption) {h}x{w}: norm64 {norm64.tolist()}, evaluator_error / bar {ratio.tolist()}")
    assert bool((ratio <= 1.0).all()) and bool((out["evaluator_error"] > 0).all())
