"""The inference kernels beyond the shipped depth-4 PReLU network, through the C ABI, against the float64 oracle: depths 1 - 6, PReLU slopes above
1 and below 0 in every layer (tests/config_weights.py, plans A / B), the parameter-free activations, state_depth < depth, the 16-bit modes at
widths with partial tiles, and the caller's buffers between guard words.  Every teacher-forced row asserts the kernels it reaches (profile names)
and that switching its route off changes the bits.  Needs a real MI355X."""
import pytest
import torch

from config_solver import DEV, _solver, _step, _unet
from config_weights import GPU_CONFIGS, config_input, config_weights
from helmnet_amd.phantoms import ring_sos_batch
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

def _cfg(tag):
    depth, seed, plan, act, sd, n, b = GPU_CONFIGS[tag]
    return dict(depth=depth, act=act, sd=sd, n=n, b=b, w=config_weights(depth, seed, plan, act, sd, n=n),
                x=config_input(n, b, depth, 9000 + n, wf_scale=1e-6))


def _oracle(c, dtype, idx):
    n, depth = c["n"], c["depth"]
    w = {k: torch.from_numpy(v).to(dtype) for k, v in c["w"].items()}
    sl = {k: torch.from_numpy(v[idx]).to(dtype) for k, v in c["x"].items()}
    st = O.unflatten_states(sl["states"], n, depth)
    d, _ = O.unet_forward(sl["x6"], st, w, depth, c["act"], state_depth=c["sd"])
    k_sq, _ = O.get_initials(sl["sos"], 1.0)
    wf, res, st2 = O.single_step(sl["wf"], k_sq, sl["res"], st, w, torch.zeros(1, 2, n, n, dtype=dtype),
                                 O.SpectralTables(n, 8, 2, 1.0, dtype=dtype), depth, c["act"], state_depth=c["sd"])
    return {"d": d, "wf": wf, "res": res, "states": O.flatten_states(st2)}


def _vs_float64(name, got, w64, w32, report):
    """L_inf <= 1e-5 * max of the float64 result, or 2 x the fp32 oracle's own distance where that is above 5e-6."""
    scale = w64.abs().max().item()
    err = (got.detach().cpu().double() - w64).abs().max().item() / scale
    ora = (w32.double() - w64).abs().max().item() / scale
    bar = 1e-5 if ora <= 5e-6 else 2 * ora
    report.append(f"{name}: {err:.2e} (fp32 oracle {ora:.2e}, bar {bar:.2e})")
    return err <= bar


def _levels(n, depth):
    o, out = 0, []
    for d in range(depth):
        out.append(slice(o, o + (n >> d) ** 2))
        o += (n >> d) ** 2
    return out


def _names(s, x):
    eng = s.engine()
    eng.profile_enable(None)
    _step(s, x)
    torch.cuda.synchronize()
    names = set(eng.profile_collect())
    eng.profile_enable([])
    eng.check_async_errors()
    return names


# tag -> (kernels it must reach, kernels it must not reach, options that switch the route off)
ROUTES = {
    "d4_256_A": ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 1), ("deep", 0), ("dc_valu", 0)]),
    "d4_256_B": ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 1), ("deep", 0), ("dc_valu", 0)]),
    "d4_256_relu": ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 0), ("dc_valu", 0)]),
    "d4_256_leakyrelu": ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 0), ("dc_valu", 0)]),
    "d4_512_A": ({"inc_conv_signal0", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}, [("deep", 0), ("dc_valu", 0)]),
    "d4_512_B": ({"inc_conv_signal0", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}, [("deep", 0), ("dc_valu", 0)]),
    "d4_256_A_b33": ({"deep", "conv_signal2"}, {"conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d3_128": ({"conv_signal0", "deep"}, {"conv_signal1", "conv_signal2", "bottleneck"}, [("deep", 1), ("deep", 0)]),
    "d3_256": ({"inc_conv_signal0", "conv_signal1", "deep"}, {"conv_signal2", "bottleneck"}, [("deep", 0), ("dc_valu", 0)]),
    "d2_128": ({"deep"}, {"conv_signal1", "bottleneck"}, [("deep", 0)]),
    "d2_64": ({"deep"}, {"conv_signal1", "bottleneck"}, [("deep", 0)]),
    "d5_512": ({"conv_signal1", "conv_signal2", "deep"}, {"conv_signal3", "conv_signal4", "bottleneck"}, [("deep", 1), ("deep", 0)]),
    "d6_256": ({f"conv_signal{d}" for d in range(1, 6)} | {"bottleneck"}, {"deep"}, [("dc_valu", 0)]),
    "d1_256": ({"inc_conv_signal0", "bottleneck"}, {"deep"}, [("dc_valu", 0)]),
    "d4_256_sd2": ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d4_512_sd0": ({"inc_conv_signal0", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d4_256_softplus": ({"inc", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d4_256_gelu": ({"inc", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d4_512_softplus": ({"inc", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}, [("deep", 0)]),
    "d4_512_gelu": ({"inc", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}, [("deep", 0)]),
    # 528 = 16 * 33: no level is 32 or 64 wide, so neither deep kernel applies (deep_applies, deepx_levels): every level layer by layer down to a 33-wide
    # bottleneck; level 0 (528 = 4 * 132 >= 256) still takes the paired hand-scheduled kernel
    "d4_528_A": ({"inc_conv_signal0", "conv_signal1", "conv_signal2", "conv_signal3", "bottleneck"}, {"deep", "inc", "conv_signal0"}, [("dc_valu", 0)]),
}


@pytest.mark.parametrize("tag", list(ROUTES))
def test_teacher_forced_step_on_every_route_vs_float64(tag):
    c = _cfg(tag)
    n, depth, sd, b = c["n"], c["depth"], c["sd"], c["b"]
    must, must_not, flips = ROUTES[tag]
    s = _solver(depth, c["act"], sd, c["w"], n)
    names = _names(s, c["x"])
    assert must <= names and not (must_not & names), (sorted(names), must, must_not)
    got = dict(zip(("wf", "res", "states"), _step(s, c["x"])))
    got["d"] = _unet(s, c["x"])
    s.engine().check_async_errors()
    idx = [0, b - 1] if b > 2 else list(range(b))      # the float64 oracle on a slice of the batch (samples are independent)
    w64, w32 = _oracle(c, torch.float64, idx), _oracle(c, torch.float32, idx)
    report, ok = [], []
    for k in ("d", "wf", "res"):
        ok.append(_vs_float64(k, got[k][idx], w64[k], w32[k], report))
    x_st = torch.from_numpy(c["x"]["states"])
    for d, lv in enumerate(_levels(n, depth)):
        if d < sd:      # each level's new state on its own scale (level 3 of 256^2 is 1 % of the flat vector)
            ok.append(_vs_float64(f"state{d}", got["states"][idx][:, :, lv], w64["states"][:, :, lv], w32["states"][:, :, lv], report))
        else:           # a level without state keeps what its slot held (architectures.py:250-251)
            assert torch.equal(got["states"][:, :, lv].cpu(), x_st[:, :, lv]), d
    print(f"[{tag}] " + "; ".join(report))
    assert all(ok), report
    # the route is not the fallback: switching it off changes the bits, within the bar between kernel sets
    base = [got["wf"], got["res"], got["states"]]
    for opt, val in flips:
        f = _solver(depth, c["act"], sd, c["w"], n)
        f.engine().set_option(opt, val)
        other = _step(f, c["x"])
        f.engine().check_async_errors()
        assert not all(torch.equal(a, o) for a, o in zip(base, other)), (opt, val)
        for a, o in zip(base, other):
            assert (a - o).abs().max().item() <= 4e-6 * o.abs().max().item(), (opt, val)
    if tag == "d4_256_A_b33":    # k_deepx stands down above 32 maps: samples 0 and 32 against the same samples in a batch of 2 (k_deepx)
        two = {k: v[[0, b - 1]] for k, v in c["x"].items()}
        pair = _step(_solver(depth, c["act"], sd, c["w"], n), two)
        for a, o in zip(base, pair):
            assert (a[[0, b - 1]] - o).abs().max().item() <= 4e-6 * o.abs().max().item()
    if sd < depth:       # NaN in the stateless slots stays out of the output and stays in its slot
        a = _levels(n, depth)[sd].start
        st = torch.from_numpy(c["x"]["states"]).clone()
        st[:, :, a:] = float("nan")
        poisoned = _step(s, c["x"], st)
        assert torch.equal(poisoned[0], got["wf"]) and torch.equal(poisoned[1], got["res"])
        assert torch.equal(poisoned[2][:, :, :a], got["states"][:, :, :a]) and torch.isnan(poisoned[2][:, :, a:]).all()


@pytest.mark.parametrize("tag,it_oracle", [("d3_128", True), ("d2_64", True), ("d5_512", False), ("d1_256", False), ("d4_256_relu", False)])
def test_loop_is_repeated_single_step_bit_for_bit(tag, it_oracle):
    """forward(sos, 30) == 30 x single_step (the configurations decide between flag-sync and event release differently); graph replay and two
    lanes give the same bits; where cheap, a float64 O.solve of the same 30 iterations (the cfg3 bar form of DESIGN section 2)."""
    c = _cfg(tag)
    n, depth, sd = c["n"], c["depth"], c["sd"]
    b = min(c["b"], 2)
    s = _solver(depth, c["act"], sd, c["w"], n, zero_source=False)
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=21)).to(DEV)
    ref = s.forward(sos, num_iterations=30, residuals="last")
    wf_ref, res_ref, st_ref = ref["wavefields"][0].clone(), ref["residuals"][-1].clone(), s.f.get_states(flatten=True).clone()
    k_sq, wf = s.get_initials(sos)
    s.f.clear_states(wf)
    res = s.get_residual(wf, k_sq)
    for _ in range(30):
        wf, res = s.single_step(wf, k_sq, res)
    assert torch.equal(wf, wf_ref) and torch.equal(res, res_ref) and torch.equal(s.f.get_states(flatten=True), st_ref)
    if tag in ("d3_128", "d2_64"):
        eng = s.engine()
        for opt, val in (("graph", 1), ("lanes", 2)):
            eng.set_option(opt, val)
            try:
                o = s.forward(sos, num_iterations=30, residuals="last")
                assert torch.equal(o["wavefields"][0], wf_ref) and torch.equal(o["residuals"][-1], res_ref), opt
                assert torch.equal(s.f.get_states(flatten=True), st_ref), opt
            finally:
                eng.set_option(opt, 1 if opt == "lanes" else 0)
    s.engine().check_async_errors()
    if it_oracle:
        src = O.point_source_map(n, [n // 8, n // 2], 10.0)
        w32 = {k: torch.from_numpy(v) for k, v in c["w"].items()}
        w64 = {k: v.double() for k, v in w32.items()}
        o32 = O.solve(sos.cpu(), w32, src, O.SpectralTables(n, 8, 2, 1.0), 30, depth=depth, act=c["act"], state_depth=sd)["wavefield"]
        o64 = O.solve(sos.cpu().double(), w64, src.double(), O.SpectralTables(n, 8, 2, 1.0, dtype=torch.float64), 30, depth=depth,
                      act=c["act"], state_depth=sd)["wavefield"]
        scale = o64.abs().max().item()
        err, ora = (wf_ref.cpu().double() - o64).abs().max().item(), (o32.double() - o64).abs().max().item()
        print(f"[{tag}] 30 it: Linf vs float64 {err:.3e}, fp32 oracle {ora:.3e}, |wf| {scale:.3e}")
        assert err <= max(1e-4 * scale, 2 * ora) and err <= 4e-4 * scale


def test_one_context_through_three_networks_and_two_domains(weights):
    """One context: checkpoint at 256^2 -> fresh depth 3 at 128^2 -> checkpoint at 256^2; each run gives the bits of a fresh context (a stale
    sigma map, workspace or graph would not)."""
    from helmnet_amd import IterativeSolver
    c3 = _cfg("d3_128")

    def ckpt():
        s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
        s.set_domain_size(256, source_location=[30, 128])
        return s

    sos256 = torch.from_numpy(ring_sos_batch(256, 2, seed=3)).to(DEV)
    sos128 = torch.from_numpy(ring_sos_batch(128, 2, seed=4)).to(DEV)
    fresh = [ckpt().forward(sos256, num_iterations=12, residuals="last")["wavefields"][0],
             _solver(3, "prelu", 3, c3["w"], 128, zero_source=False).forward(sos128, num_iterations=12, residuals="last")["wavefields"][0]]
    s = ckpt()
    eng = s.engine()
    runs = [s.forward(sos256, num_iterations=12, residuals="last")["wavefields"][0].clone()]
    s.hparams.depth, s.hparams.state_depth = 3, 3
    s.init_f()
    s.f.load_state_dict({k: torch.from_numpy(v) for k, v in c3["w"].items()}, strict=True)
    s.set_domain_size(128, source_location=[16, 64])
    runs.append(s.forward(sos128, num_iterations=12, residuals="last")["wavefields"][0].clone())
    s.hparams.depth, s.hparams.state_depth = 4, 4
    s.init_f()
    s.f.load_state_dict(weights, strict=True)
    s.set_domain_size(256, source_location=[30, 128])
    runs.append(s.forward(sos256, num_iterations=12, residuals="last")["wavefields"][0].clone())
    assert s.engine() is eng
    assert torch.equal(runs[0], fresh[0]) and torch.equal(runs[1], fresh[1]) and torch.equal(runs[2], fresh[0])


@pytest.mark.parametrize("tag", ["d4_272_A", "d4_512_A16"])
def test_16_bit_modes_at_partial_tiles_and_512_vs_float64(tag):
    """bf16x3 / bf16x2 / fp16 (k_dc_x16, k_down_x16, k_up_x16) at 272^2 (level 1 is 136 wide: partial tiles both ways) and 512^2 against the
    float64 oracle, with each mode's bar of test_gpu_parity.py; each differs from the fp32 mode, so the 16-bit kernels ran."""
    c = _cfg(tag)
    n, b = c["n"], c["b"]
    idx = list(range(b))
    w64, w32 = _oracle(c, torch.float64, idx), _oracle(c, torch.float32, idx)
    scale = w64["d"].abs().max().item()
    ora = (w32["d"].double() - w64["d"]).abs().max().item() / scale
    outs = {}
    for mode in ("fp32", "bf16x3", "bf16x2", "fp16"):
        s = _solver(4, "prelu", 4, c["w"], n, mode=mode)
        assert s.engine().unet_precision == mode
        outs[mode] = _unet(s, c["x"]).cpu()
        s.engine().check_async_errors()
    err = {m: (o.double() - w64["d"]).abs().max().item() / scale for m, o in outs.items()}
    print(f"[{tag}] d vs float64: {err}, fp32 oracle {ora:.2e}")
    assert err["fp32"] <= max(1e-5, 2 * ora)
    assert err["bf16x3"] <= 1e-5 and err["bf16x3"] <= 1.25 * ora
    assert err["bf16x2"] <= 1e-4 and err["fp16"] <= 5e-3
    for m in ("bf16x3", "bf16x2", "fp16"):
        assert not torch.equal(outs[m], outs["fp32"]), m


PAYLOAD = 0x7FC0BEEF    # a quiet NaN with a payload of its own


def _guarded(t, margin):
    buf = torch.empty(2 * margin + t.numel(), dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(PAYLOAD)
    view = buf[margin:margin + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.parametrize("n,b,mode", [(256, 3, "fp32"), (272, 3, "fp32"), (272, 3, "fp16"), (512, 1, "fp32"), (96, 2, "fp32")])
def test_caller_buffers_between_guard_words(n, b, mode):
    """Engine.step on views inside larger buffers whose margins (a plane each side) hold a NaN payload: the same bits as plain tensors, and
    every guard word intact afterwards (an out-of-bounds read would bring NaN in, a write would overwrite the payload)."""
    w = config_weights(4, 749, "A", n=n)
    s = _solver(4, "prelu", 4, w, n, mode=mode, zero_source=False)
    eng = s.engine()
    x = config_input(n, b, 4, 9100 + n, wf_scale=0.5)
    K = 3
    k_sq = (1.0 / torch.from_numpy(x["sos"])) ** 2
    ins = {"wf": torch.from_numpy(x["wf"]), "res": torch.from_numpy(x["res"]), "states": torch.from_numpy(x["states"]), "k_sq": k_sq,
           "src": s._src().cpu(), "res_hist": torch.zeros(K, b, 2, n, n), "wf_hist": torch.zeros(K, b, 2, n, n),
           "st_hist": torch.zeros(K, b, 2, eng.state_len), "rmse_hist": torch.zeros(K, b)}
    plain = {k: v.to(DEV).contiguous() for k, v in ins.items()}
    order = ("wf", "res", "states", "k_sq", "src")
    eng.step(*[plain[k] for k in order], K, plain["res_hist"], plain["wf_hist"], plain["st_hist"], plain["rmse_hist"])
    margin = n * n
    bufs, views = {}, {}
    for k, v in ins.items():
        bufs[k], views[k] = _guarded(v.to(DEV), margin)
    eng.step(*[views[k] for k in order], K, views["res_hist"], views["wf_hist"], views["st_hist"], views["rmse_hist"])
    torch.cuda.synchronize()
    eng.check_async_errors()
    for k in ins:
        if k == "rmse_hist":     # per-sample sums of float atomics: order-dependent in the last bits
            assert torch.allclose(views[k], plain[k], rtol=1e-5, atol=0), k
        else:
            assert torch.equal(views[k], plain[k]), k
        g = bufs[k].view(torch.int32)
        assert (g[:margin] == PAYLOAD).all() and (g[-margin:] == PAYLOAD).all(), k


@pytest.mark.parametrize("n,b", [(256, 5), (512, 3)])
def test_a_poisoned_sample_leaves_the_others_alone(n, b):
    """A NaN in one pixel of sample 2: every other sample's wavefield, residual and states keep their bits, its RMSE row its value; sample 2 is
    non-finite."""
    w = config_weights(4, 749, "A", n=n)
    s = _solver(4, "prelu", 4, w, n, zero_source=False)
    eng = s.engine()
    x = config_input(n, b, 4, 9200 + n, wf_scale=0.5)
    k_sq = ((1.0 / torch.from_numpy(x["sos"])) ** 2).to(DEV)
    out = {}
    for poison in (False, True):
        wf = torch.from_numpy(x["wf"]).to(DEV)
        if poison:
            wf[2, 0, n // 2, n // 3] = float("nan")
        res, st = torch.from_numpy(x["res"]).to(DEV), torch.from_numpy(x["states"]).to(DEV)
        rm = torch.zeros(2, b, device=DEV)
        eng.step(wf, res, st, k_sq, s._src(), 2, rmse_hist=rm)
        out[poison] = (wf, res, st, rm)
    torch.cuda.synchronize()
    eng.check_async_errors()
    keep = [i for i in range(b) if i != 2]
    for a, p in zip(out[False][:3], out[True][:3]):
        assert torch.equal(a[keep], p[keep])
    assert torch.allclose(out[False][3][:, keep], out[True][3][:, keep], rtol=1e-5, atol=0)
    assert not torch.isfinite(out[True][0][2]).all() and not torch.isfinite(out[True][3][:, 2]).all()
