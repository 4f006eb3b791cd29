"""GPU: the four planning kernels (vj_plan.hip) through their ops wrappers, against the reference planner's
recorded results (tests/golden/planning.pt), the same expressions in torch f32 where the kernel is meant to be
bitwise, and float64 recomputations with derived bounds elsewhere. Outputs live inside guard bands that must
stay untouched; inputs are strided where the entry point takes a stride."""

import math

import pytest
import torch

import planning_fixture as fx

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0**-24  # f32 unit roundoff
SENTINEL = -777.25


def guarded(shape, dtype=torch.float32, pad=96):
    """(whole buffer, view of `shape` in its middle); check_guards(buf) after the call."""
    n = math.prod(shape)
    buf = torch.full((pad + n + pad,), int(SENTINEL) if dtype == torch.int32 else SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n].view(*shape)


def check_guards(buf, pad=96):
    want = int(SENTINEL) if buf.dtype == torch.int32 else SENTINEL
    assert bool((buf[:pad] == want).all()) and bool((buf[-pad:] == want).all()), "guard band written"


# ------------------------------------------------------------------------------------------------ cem_sample
def sample_ref(noise, mean, std, maxnorm, axis, close_from):
    """mpc_utils.py:93-107 in torch f32 on the CPU, one rollout step after the other."""
    rollout, S, _ = noise.shape
    out = torch.zeros(S, rollout, 7)
    for h in range(rollout):
        a = noise[h] * std[h] + mean[h]
        a[:, :3] = torch.clip(a[:, :3], min=-maxnorm, max=maxnorm)
        a[:, -1:] = torch.clip(a[:, -1:], min=-0.75, max=0.75)
        for ax in axis.keys():
            a[:, ax] = axis[ax]
        out[:, h, :3] = a[:, :3]
        out[:, h, 6] = a[:, 3]
        if close_from is not None and h >= close_from:
            out[:, h, 6] = 1.0
    return out


def run_sample(noise, mean, std, maxnorm, axis, close_from):
    from vjepa2_amd import ops

    rollout, S, _ = noise.shape
    buf, out = guarded((S, rollout, 7))
    ops.cem_sample(noise.to(DEV), mean.to(DEV), std.to(DEV), maxnorm, axis=axis, close_from=close_from, out=out)
    check_guards(buf)
    return out.cpu()


@pytest.mark.parametrize("rollout", [1, 2, 3])
@pytest.mark.parametrize("S", [2, 16, 65, 400])
def test_cem_sample_bitwise_vs_torch_f32(S, rollout):
    g = torch.Generator().manual_seed(S * 10 + rollout)
    noise = torch.randn(rollout, S, 4, generator=g)
    mean = 0.03 * torch.randn(rollout, 4, generator=g)
    std = torch.rand(rollout, 4, generator=g) * torch.tensor([0.05, 0.05, 0.05, 1.0])
    for axis in ({}, {1: 0.01}, {0: -0.02, 3: 0.5}):
        for close_from in (None, 0, 1):
            got = run_sample(noise, mean, std, 0.05, axis, close_from)
            want = sample_ref(noise, mean, std, 0.05, axis, close_from)
            assert torch.equal(got, want), (axis, close_from, (got - want).abs().max().item())
            assert not got[:, :, 3:6].any()


def test_cem_sample_zero_std_and_all_clips_active():
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(2, 33, 4, generator=g)
    mean = torch.tensor([[0.01, -0.02, 0.03, 0.4], [0.2, -0.2, 0.0, -0.9]])
    got = run_sample(noise, mean, torch.zeros(2, 4), 0.05, {}, None)
    want = sample_ref(noise, mean, torch.zeros(2, 4), 0.05, {}, None)
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0], torch.tensor([0.01, -0.02, 0.03, 0, 0, 0, 0.4]))
    assert torch.equal(got[0, 1], torch.tensor([0.05, -0.05, 0.0, 0, 0, 0, -0.75]))
    big = noise * 100 + torch.sign(noise)  # |noise * std + mean| >= 0.9 everywhere: every clip is active
    std, mean = torch.ones(2, 4), 0.1 * torch.sign(mean)
    got = run_sample(big, mean, std, 0.05, {}, None)
    assert torch.equal(got, sample_ref(big, mean, std, 0.05, {}, None))
    assert torch.equal(got[:, :, :3].abs(), torch.full((33, 2, 3), 0.05))
    assert torch.equal(got[:, :, 6].abs(), torch.full((33, 2), 0.75))


def test_cem_sample_matches_reference_recordings():
    """Bitwise: the recorded noise, mean and std of every iteration of every run give the recorded actions."""
    c = fx.load()["cem"]
    for name, run in c["runs"].items():
        axis = {a: v for a, v in run["axis"]}
        f = run["f32"]
        for it in range(run["cem_steps"]):
            got = run_sample(f["noise"][it], f["mean"][it], f["std"][it], c["mpc"]["maxnorm"], axis,
                             run["close_gripper"])
            assert torch.equal(got, f["actions"][it]), (name, it, (got - f["actions"][it]).abs().max().item())


# ------------------------------------------------------------------------------------------------ pose_step
def test_pose_step_matches_reference():
    """xyz and gripper bitwise (one f32 add, one clip); angles within 2^-22: both sides are f64 results rounded
    once to f32 and the magnitudes are below 4, so they differ by at most one ulp <= 2^-22."""
    from vjepa2_amd import ops

    p = fx.load()["pose"]
    n = p["pose"].shape[0]
    pose = torch.full((n, 9), 3.0, device=DEV)  # row strides 9 / 8 / 10: the entry point takes them
    act = torch.full((n, 8), 3.0, device=DEV)
    pose[:, :7], act[:, :7] = p["pose"].to(DEV), p["action"].to(DEV)
    buf, out = guarded((n, 10))
    ops.pose_step(pose[:, :7], act[:, :7], out=out[:, :7])
    check_guards(buf)
    assert bool((out[:, 7:] == SENTINEL).all())  # the columns between two rows stay untouched too
    got, want = out[:, :7].cpu(), p["new_pose"]
    assert torch.equal(got[:, :3], want[:, :3]) and torch.equal(got[:, 6], want[:, 6])
    assert want[:, 3:6].abs().max().item() < 4
    err = (got[:, 3:6].double() - want[:, 3:6].double()).abs().max().item()
    assert err <= 2.0**-22, err
    got2 = ops.pose_step(p["pose"].to(DEV), p["action"].to(DEV)).cpu()  # contiguous rows, allocated output
    assert torch.equal(got2, got)


# ------------------------------------------------------------------------------------------------ plan_frame
def frame_ref(x, goal, normalize):
    """float64 layer_norm (no affine, eps 1e-5) + mean |y - goal|, with the per-element / per-sample bounds of an
    f32 evaluation in the kernel's summation shape (a lane adds 4 * ceil(D / 256) <= 32 terms, then a 6-level
    tree; the rows of a sample are combined in f64):
      mean:  |dm| <= (L + 2) u mean|x|, L = 4 ceil(D / 256) + 6 (the sum, 1 / D and the product)
      rstd:  relative (L + 4) / 2 u (the variance sum on rounded differences) + 3 u (add, sqrt, divide)
      y:     |dy| <= rstd |dm| + |y| (2 u + rel(rstd))
      e:     mean |dy| + (L + 2) u e
    doubled for the second-order terms dropped above. Without normalisation y = x exactly."""
    S, R, D = x.shape
    L = 4 * -(-D // 256) + 6
    x64 = x.double()
    if normalize:
        m = x64.mean(-1, keepdim=True)
        var = x64.var(-1, unbiased=False, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        y = (x64 - m) * rstd
        by = 2 * (rstd * (L + 2) * U * x64.abs().mean(-1, keepdim=True) + y.abs() * ((L + 4) / 2 + 5) * U)
    else:
        y, by = x64, torch.zeros_like(x64)
    e = (y - goal.double()[None]).abs().mean(dim=(1, 2))
    be = by.mean(dim=(1, 2)) + 2 * (L + 2) * U * e
    return y, by, e, be


@pytest.mark.parametrize("S", [1, 2, 65])
@pytest.mark.parametrize("R,D", [(1, 96), (4, 96), (3, 1024), (256, 1408)])
def test_plan_frame_vs_float64(R, D, S):
    """Every combination of normalise / dst / energy on the last frame of a 2-frame (3 for the small shapes)
    sequence, i.e. a source whose sample stride exceeds R * D; sample 0's row 0 has zero variance."""
    from vjepa2_amd import ops

    g = torch.Generator(device=DEV).manual_seed(R * 7 + D + S)
    T = 2 if R * D > 4096 else 3
    seq = torch.randn(S, T, R, D, device=DEV, generator=g) * 1.7 + 0.3
    seq[0, -1, 0] = 0.7  # a constant row: variance 0, no NaN
    src = seq[:, -1]
    assert src.stride(0) == T * R * D
    goal = torch.randn(R, D, device=DEV, generator=g)
    seq0 = seq.clone()
    for normalize in (True, False):
        y, by, e, be = frame_ref(src, goal, normalize)
        for want_dst in (True, False):
            for want_e in (True, False):
                if not (want_dst or want_e):
                    continue
                dbuf, dwhole = guarded((S, 2, R, D))  # the dst sample stride is 2 R D: slot 1 of a trajectory
                dst = dwhole[:, 1] if want_dst else None
                ebuf, en = guarded((S,))
                out = ops.plan_frame(src, goal=goal if want_e else None, dst=dst, normalize=normalize,
                                     energy=en if want_e else None)
                check_guards(dbuf), check_guards(ebuf)
                assert bool((dwhole[:, 0] == SENTINEL).all())  # slot 0 of every sample is not this call's
                if want_dst:
                    assert out[0] is dst and torch.isfinite(dst).all()
                    err = (dst.double() - y).abs()
                    assert bool((err <= by).all()), (normalize, (err - by).max().item())
                    if not normalize:
                        assert torch.equal(dst, src)
                else:
                    assert bool((dwhole == SENTINEL).all())
                if want_e:
                    assert torch.isfinite(en).all()
                    err = (en.double() - e).abs()
                    assert bool((err <= be).all()), (normalize, err.max().item(), be.min().item())
                else:
                    assert out[1] is None and bool((en == SENTINEL).all())
    assert torch.equal(seq, seq0)  # the source is read only


# ------------------------------------------------------------------------------------------------ cem_update
MOM = dict(momentum_mean=0.15, momentum_std=0.25, momentum_mean_gripper=0.1, momentum_std_gripper=0.3)
COLS = [0, 1, 2, 6]


def update_ref(energy, actions, k, mean, std, mom):
    """float64: stable argsort (ties: lower index first, NaN last), mean / unbiased std over the elites, the
    momentum update; and the bound of an f32 evaluation: two scalar roundings, two products and one sum are 4 u
    per term, 1 u more for the rounded statistic; the mean is an f32 sum of k terms ((k - 1) u mean|v|, whatever
    the order), the std is formed in f64 and rounded once."""
    e = energy.double().clone()
    e[e.isnan()] = float("inf")
    order = torch.sort(e, stable=True).indices[:k]
    elites = torch.sort(order).values
    sel = actions.double()[elites][:, :, COLS]  # [k, rollout, 4]
    m, s = sel.mean(0), sel.std(0, unbiased=True)
    mm = torch.tensor([mom["momentum_mean"]] * 3 + [mom["momentum_mean_gripper"]], dtype=torch.float64)
    ms = torch.tensor([mom["momentum_std"]] * 3 + [mom["momentum_std_gripper"]], dtype=torch.float64)
    new_mean = m * (1 - mm) + mean.double() * mm
    new_std = s * (1 - ms) + std.double() * ms
    b_mean = U * ((k - 1) * sel.abs().mean(0) * (1 - mm) + 5 * ((m * (1 - mm)).abs() + (mean.double() * mm).abs()))
    b_std = 5 * U * ((s * (1 - ms)).abs() + (std.double() * ms).abs())
    return elites.to(torch.int32), new_mean, new_std, b_mean, b_std


def run_update(energy, actions, k, mean, std, mom=MOM):
    from vjepa2_amd import ops

    rollout = actions.shape[1]
    mbuf, m = guarded((rollout, 4))
    sbuf, s = guarded((rollout, 4))
    ibuf, idx = guarded((k,), dtype=torch.int32)
    m.copy_(mean), s.copy_(std)
    a0 = actions.to(DEV)
    a1 = a0.clone()
    ops.cem_update(energy.to(DEV), a1, k, m, s, elite_idx=idx, **mom)
    check_guards(mbuf), check_guards(sbuf), check_guards(ibuf)
    assert torch.equal(a0, a1)
    return idx.cpu(), m.cpu(), s.cpu()


def check_update(energy, actions, k, mean, std, mom=MOM):
    idx, m, s = run_update(energy, actions, k, mean, std, mom)
    elites, rm, rs, bm, bs = update_ref(energy, actions, k, mean, std, mom)
    assert torch.equal(idx, elites), (idx.tolist()[:12], elites.tolist()[:12])
    assert bool(((m.double() - rm).abs() <= bm).all()), ((m.double() - rm).abs().max().item(), bm.min().item())
    assert bool(((s.double() - rs).abs() <= bs).all()), ((s.double() - rs).abs().max().item(), bs.min().item())
    return idx, m, s


@pytest.mark.parametrize("S", [2, 10, 64, 65, 400, 4096])
def test_cem_update_vs_float64(S):
    g = torch.Generator().manual_seed(S)
    for rollout in (1, 3):
        for k in sorted({2, min(10, S), S}):
            energy = torch.rand(S, generator=g) + 0.5
            actions = torch.randn(S, rollout, 7, generator=g) * torch.tensor([.05, .05, .05, 9, 9, 9, .7])
            mean = 0.02 * torch.randn(rollout, 4, generator=g)
            std = torch.rand(rollout, 4, generator=g) + 0.01
            check_update(energy, actions, k, mean, std)


def test_cem_update_ties_go_to_the_lower_index_and_nan_ranks_last():
    g = torch.Generator().manual_seed(3)
    S = 130
    actions = torch.randn(S, 2, 7, generator=g)
    mean, std = torch.zeros(2, 4), torch.ones(2, 4)
    energy = torch.full((S,), 2.0)
    energy[[7, 70, 129]] = 1.0  # three clear winners, then a 127-way tie for the rest
    idx, _, _ = check_update(energy, actions, 6, mean, std)
    assert idx.tolist() == [0, 1, 2, 7, 70, 129]
    energy = torch.rand(S, generator=g)
    energy[[0, 1, 64, 65, 128]] = float("nan")  # NaNs at low indices and at wave edges
    for k in (2, 64, S - 5):
        idx, m, s = check_update(energy, actions, k, mean, std)
        assert not set(idx.tolist()) & {0, 1, 64, 65, 128}
        assert torch.isfinite(m).all() and torch.isfinite(s).all()
    energy[5] = float("-inf")
    energy[6] = float("inf")
    idx, _, _ = check_update(energy, actions, 3, mean, std)
    assert 5 in idx.tolist() and 6 not in idx.tolist()


def test_cem_update_constant_column_gives_exactly_zero_std():
    g = torch.Generator().manual_seed(4)
    S, k = 400, 10
    energy = torch.rand(S, generator=g)
    actions = torch.randn(S, 2, 7, generator=g)
    actions[:, 1, 6] = 1.0  # close_gripper
    actions[:, 0, 1] = 0.01  # an axis override: not a power of two
    mean, std = torch.zeros(2, 4), torch.rand(2, 4, generator=g) + 0.5
    _, m, s = check_update(energy, actions, k, mean, std)
    take_g = torch.tensor(MOM["momentum_std_gripper"], dtype=torch.float32)
    take = torch.tensor(MOM["momentum_std"], dtype=torch.float32)
    assert s[1, 3].item() == (std[1, 3] * take_g).item()  # 0.0 * (1 - m) + std * m, exactly
    assert s[0, 1].item() == (std[0, 1] * take).item()
    keep_g = torch.tensor(1.0 - MOM["momentum_mean_gripper"], dtype=torch.float32)
    assert m[1, 3].item() == (torch.tensor(1.0) * keep_g).item()


def test_cem_update_swapped_momenta_would_show():
    """The four momenta are distinct: the update with any two of them exchanged is outside the bound."""
    g = torch.Generator().manual_seed(6)
    S, k = 64, 10
    energy = torch.rand(S, generator=g)
    actions = torch.randn(S, 1, 7, generator=g)
    mean, std = torch.randn(1, 4, generator=g), torch.rand(1, 4, generator=g) + 1
    _, m, s = check_update(energy, actions, k, mean, std)
    names = list(MOM)
    for i in range(4):
        for j in range(i + 1, 4):
            sw = dict(MOM)
            sw[names[i]], sw[names[j]] = MOM[names[j]], MOM[names[i]]
            _, rm, rs, bm, bs = update_ref(energy, actions, k, mean, std, sw)
            assert not (bool(((m.double() - rm).abs() <= bm).all()) and bool(((s.double() - rs).abs() <= bs).all()))


def test_cem_update_matches_reference_recordings():
    """Every iteration of every run: the elite set is the reference's, and mean / std after the update are within
    the same f32 bound of the reference's mean / std at the next iteration's draw (its std comes from an f64
    accumulation too; 2 u more for its own rounding of the two statistics)."""
    c = fx.load()["cem"]
    k = c["mpc"]["topk"]
    mom = {n: c["mpc"][n] for n in MOM}
    for name, run in c["runs"].items():
        f = run["f32"]
        for it in range(run["cem_steps"]):
            idx, m, s = check_update(f["energy"][it], f["actions"][it], k, f["mean"][it], f["std"][it], mom)
            assert torch.equal(idx, f["elites"][it]), (name, it)
            if it + 1 < run["cem_steps"]:
                _, rm, rs, bm, bs = update_ref(f["energy"][it], f["actions"][it], k, f["mean"][it], f["std"][it], mom)
                bm, bs = bm + 2 * U * rm.abs(), bs + 2 * U * rs.abs()
                for ref32, ref64, b in ((f["mean"][it + 1], rm, bm), (f["std"][it + 1], rs, bs)):
                    assert bool(((ref32.double() - ref64).abs() <= b).all()), (name, it, "reference outside its bound")
                assert bool(((m.double() - f["mean"][it + 1].double()).abs() <= bm).all()), (name, it)
                assert bool(((s.double() - f["std"][it + 1].double()).abs() <= bs).all()), (name, it)


# ------------------------------------------------------------------------------------------------ determinism
def test_kernels_are_bitwise_reproducible_and_stream_safe():
    from vjepa2_amd import ops

    g = torch.Generator(device=DEV).manual_seed(9)
    S, rollout, R, D, k = 400, 2, 4, 96, 10
    noise = torch.randn(rollout, S, 4, device=DEV, generator=g)
    mean0 = 0.01 * torch.randn(rollout, 4, device=DEV, generator=g)
    std0 = torch.rand(rollout, 4, device=DEV, generator=g)
    seq = torch.randn(S, 2, R, D, device=DEV, generator=g)
    goal = torch.randn(R, D, device=DEV, generator=g)
    pose = torch.randn(S, 7, device=DEV, generator=g)

    def once():
        actions = ops.cem_sample(noise, mean0, std0, 0.05, axis={1: 0.01}, close_from=1)
        new_pose = ops.pose_step(pose, actions[:, 0] + 0.3)
        dst, energy = ops.plan_frame(seq[:, -1], goal=goal, dst=torch.empty(S, R, D, device=DEV))
        mean, std = mean0.clone(), std0.clone()
        idx = ops.cem_update(energy, actions, k, mean, std, want_idx=True)
        return [actions, new_pose, dst, energy, mean, std, idx]

    a = once()
    b = once()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = once()
    torch.cuda.current_stream().wait_stream(side)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
