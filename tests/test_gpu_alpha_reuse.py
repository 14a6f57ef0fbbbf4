"""The fragment-reuse form of the N = 1024 BF16X3 coupling GEMM
(coupling_gemm_bf16x3_shift, kura_kernels.hip): bit for bit the general
form and the oracle, on the GEMM alone and through reset + step, and never
taken by an alpha without the grid's shift structure.

KURA_ALPHA_REUSE=0 (read by libkura on every kura_set_coupling /
kura_selftest_coupling) forces the general form in the same binary."""
from __future__ import annotations

import copy
import importlib
import os

import numpy as np
import pytest

from helpers import actions, make_case, ko

pytestmark = pytest.mark.gpu
N = 1024
STEPS = 3


@pytest.fixture(scope="module")
def torch_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def lib(torch_gpu):
    return importlib.import_module("dbs-gym_amd.abi").load_library()


class general_form:
    """KURA_ALPHA_REUSE=0 for the calls inside (the variable is restored)."""

    def __enter__(self):
        self.old = os.environ.get("KURA_ALPHA_REUSE")
        os.environ["KURA_ALPHA_REUSE"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["KURA_ALPHA_REUSE"]
        else:
            os.environ["KURA_ALPHA_REUSE"] = self.old


@pytest.fixture(scope="module")
def case20():
    """env0 at N = 1024, 20 envs (a full workgroup and a padded second one)."""
    return make_case("env0", N, 20)


def perturbed(alpha):
    """One element changed inside fragment (jt, b) = (5, 10), which the reuse
    form would take from (4, 8)."""
    p = alpha.copy()
    p[32 * 5 + 5, 16 * 10 + 3] = np.float32(p[32 * 5 + 5, 16 * 10 + 3] + 0.25)
    return p


def random_symmetric(seed=7):
    a = np.random.default_rng(seed).uniform(-1, 1, (N, N)).astype(np.float32)
    return np.ascontiguousarray(np.triu(a) + np.triu(a, 1).T)


def selftest(lib, X, A):
    Y = np.zeros((32, N), np.float32)
    assert lib.kura_selftest_coupling(X.ctypes.data, A.ctypes.data, Y.ctypes.data, N, 2) == 0, lib.kura_last_error()
    return Y.view(np.uint32), lib.kura_selftest_alpha_reuse()


@pytest.mark.parametrize("which", ["grid", "perturbed"])
def test_gemm_three_way(lib, case20, which):
    """One workgroup, one 32 x 1024 operand: reuse allowed == reuse forced off
    == oracle_split_gemm_rows; the grid alpha takes the reuse form, the
    perturbed one the general form."""
    alpha = np.ascontiguousarray(case20[1])
    A = alpha if which == "grid" else perturbed(alpha)
    X = np.random.default_rng(11).uniform(-1, 1, (32, N)).astype(np.float32)
    y_on, path_on = selftest(lib, X, A)
    with general_form():
        y_off, path_off = selftest(lib, X, A)
    assert path_on == (1 if which == "grid" else 0)
    assert path_off == 0
    assert np.array_equal(y_on, y_off)
    assert np.array_equal(y_on, ko.split_gemm_rows(X, A).view(np.uint32))


def _run_sim(torch, case, B, steps):
    """reset + steps of the first B envs of case on the GPU: (reuse flag, per-step outputs, final state)."""
    sim_mod = importlib.import_module("dbs-gym_amd.sim")
    cfg, alpha, omega, gs, gr, th0, ct, st, _ = case
    c = copy.copy(cfg)
    c.n_envs = B
    sim = sim_mod.KuraSim(c, 0)
    sim.set_coupling(alpha)
    sim.set_env_params(omega[:B], gs[:B], gr[:B])
    sim.set_spectral(ct, st)
    reuse = sim.alpha_reuse()
    out = [dict(obs=sim.reset(torch.from_numpy(th0[:B])).cpu().numpy().copy())]
    for k in range(steps):
        sim.step(torch.from_numpy(actions("rand", 20, c.n_elec, k)[:B]))
        torch.cuda.synchronize()
        assert not sim.flags.cpu().numpy().any()
        out.append({n: getattr(sim, n).cpu().numpy().copy()
                    for n in ("obs", "reward", "done", "nsamp", "lfp_true", "lfp_rec")})
    state = sim.get_state()
    sim.close()
    return reuse, out, state


def _same(a, b, where):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (where, k)


@pytest.fixture(scope="module")
def oracle16(case20):
    """The oracle's reset + STEPS steps of the first 16 envs, run once."""
    cfg, alpha, omega, gs, gr, th0, ct, st, _ = case20
    c = copy.copy(cfg)
    c.n_envs = 16
    o = ko.Oracle(c, alpha)
    o.set_env_params(omega[:16], gs[:16], gr[:16])
    o.set_spectral(ct, st)
    out = [dict(obs=o.reset(th0[:16]).copy())]
    after_reset = o.state()
    for k in range(STEPS):
        r = o.step(actions("rand", 20, c.n_elec, k)[:16])
        out.append({n: r[n].copy() for n in ("obs", "reward", "done", "nsamp", "lfp_true", "lfp_rec")})
    state = o.state()
    o.close()
    return out, state, after_reset


@pytest.mark.parametrize("B", [16, 20])
def test_reset_and_steps_on_equals_off(torch_gpu, case20, oracle16, B):
    """reset + 3 steps of env0: obs, reward, done, LFP and the state bitwise
    equal between the two forms; B = 16 also equal to the oracle."""
    reuse_on, out_on, st_on = _run_sim(torch_gpu, case20, B, STEPS)
    with general_form():
        reuse_off, out_off, st_off = _run_sim(torch_gpu, case20, B, STEPS)
    assert reuse_on and not reuse_off
    for k, (a, b) in enumerate(zip(out_on, out_off)):
        _same(a, b, f"on/off, launch {k}")
    _same(st_on, st_off, "on/off, state")
    if B == 16:
        ref_out, ref_state, _ = oracle16
        for k, (a, b) in enumerate(zip(out_on, ref_out)):
            _same(a, b, f"oracle, launch {k}")
        _same(st_on, ref_state, "oracle, state")


def test_random_alpha_takes_the_general_form(torch_gpu, case20, oracle16):
    """One step of 4 envs on a random symmetric alpha, from the state the
    grid alpha's reset left: the general form, bitwise the oracle."""
    torch = torch_gpu
    sim_mod = importlib.import_module("dbs-gym_amd.sim")
    cfg, _, omega, gs, gr, th0, ct, st, _ = case20
    B = 4
    c = copy.copy(cfg)
    c.n_envs = B
    alpha = random_symmetric()
    start = {k: v[:B] for k, v in oracle16[2].items()}
    a = actions("rand", 20, c.n_elec, 0)[:B]
    o = ko.Oracle(c, alpha)
    o.set_env_params(omega[:B], gs[:B], gr[:B])
    o.set_spectral(ct, st)
    o.set_state(start)
    ref = o.step(a)
    ref_state = o.state()
    assert not o.flags.any()
    o.close()
    sim = sim_mod.KuraSim(c, 0)
    sim.set_coupling(alpha)
    assert not sim.alpha_reuse()
    sim.set_env_params(omega[:B], gs[:B], gr[:B])
    sim.set_spectral(ct, st)
    sim.set_state(start)
    sim.step(torch.from_numpy(a))
    torch.cuda.synchronize()
    assert not sim.flags.cpu().numpy().any()
    got = {n: getattr(sim, n).cpu().numpy() for n in ("obs", "reward", "done", "nsamp", "lfp_true", "lfp_rec")}
    _same(got, {n: ref[n] for n in got}, "random alpha, step")
    _same(sim.get_state(), ref_state, "random alpha, state")
    sim.close()
