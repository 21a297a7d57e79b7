"""What the GPU tests of networks other than the shipped one share: a frozen IterativeSolver around a given state dict, one teacher-forced step and one
network evaluation on config_input-style arrays (tests/test_config_matrix.py, tests/test_x16_gpu.py)."""
import torch

DEV = "cuda:0"


def _solver(depth, act="prelu", state_depth=None, weights=None, n=256, mode=None, zero_source=True):
    from helmnet_amd import IterativeSolver
    from helmnet_amd.checkpoint import default_exported_weights, read_exported_weights
    hp, _ = read_exported_weights(*default_exported_weights())
    hp.update(depth=depth, activation_function=act, state_depth=depth if state_depth is None else state_depth)
    s = IterativeSolver(**hp)
    s.f.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    s.freeze()
    s.to(DEV)
    s.set_domain_size(n, source_location=[n // 8, n // 2])
    if zero_source:   # the residual then measures L(wf) + k^2 wf alone, not a point source of amplitude 10
        s.set_source_maps(torch.zeros(1, 2, n, n, device=DEV))
    if mode is not None:
        s.set_unet_precision(mode)
    s.engine()
    return s


def _step(s, x, states=None):
    """One teacher-forced single_step (the hn_step route) -> wf, res, flat new states (device tensors)."""
    g = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    k_sq, _ = s.get_initials(g["sos"])
    s.f.set_states(g["states"] if states is None else states.to(DEV), flatten=True)
    wf, res = s.single_step(g["wf"], k_sq, g["res"])
    return wf, res, s.f.get_states(flatten=True).clone()


def _unet(s, x):
    s.f.set_states(torch.from_numpy(x["states"]).to(DEV), flatten=True)
    return s.f(torch.from_numpy(x["x6"]).to(DEV))
