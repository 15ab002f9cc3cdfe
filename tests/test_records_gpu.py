"""Game records on the device: oth_records_gpu must be bit-identical to oth_records_cpu (the
same replay code, csrc/records.h; tests/test_records_cpu.py checks the host side against the
reference), az_records_vote_gpu must equal its NumPy mirror (checked there against
remove_conflicting_duplicates), and the rows must train: replay -> dedup ->
DeviceReplayLoader.from_bitboards -> supervised_epoch."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

nat = pytest.importorskip("az_native")
import records as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("records_cases.npz")


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def both(acts, own0=None, opp0=None, winner=None, max_rows=None, flags=0):
    """(host, device) raw outputs of the same call, the device's copied back"""
    acts = np.ascontiguousarray(acts, np.uint8)
    max_rows = acts.shape[1] if max_rows is None else max_rows
    cpu = R.replay_cpu_raw(acts, own0, opp0, winner, max_rows, flags)
    gpu = R.replay_gpu_raw(dev(acts), dev(own0), dev(opp0), dev(winner), max_rows, flags)
    torch.cuda.synchronize()
    gpu = {k: v.cpu().numpy() for k, v in gpu.items()}
    for k in ("own", "opp", "final_own", "final_opp"):
        gpu[k] = gpu[k].view(np.uint64)
    return cpu, gpu


def assert_identical(cpu, gpu):
    assert set(cpu) == set(gpu) == set(R._ORDER)
    for k in R._ORDER:
        assert cpu[k].dtype == gpu[k].dtype and cpu[k].shape == gpu[k].shape, k
        assert (cpu[k] == gpu[k]).all(), k


def test_fixture_games_bit_identical(gold):
    pad = lambda a: np.pad(a, ((0, 0), (0, 16)), constant_values=255)  # noqa: E731
    acts = np.concatenate([pad(gold["free_acts"]), pad(gold["trunc_acts"]),
                           gold["pass_acts_explicit"], gold["pass_acts_omitted"]])
    winner = np.concatenate([gold["free_winner"], gold["trunc_winner"], gold["pass_winner"],
                             gold["pass_winner"]])
    for flags in (0, 1):
        for w in (None, winner):
            cpu, gpu = both(acts, winner=w, flags=flags)
            assert_identical(cpu, gpu)
            assert (cpu["n_rows"][:64] == gold["free_len"]).all()


@pytest.fixture(scope="module")
def mixed():
    """4,099 random playouts with every pass written (stride 80): a third finished, a third
    cut short, a third with one entry overwritten by a random byte; and the same games resumed
    from their position after four plies."""
    n = 4099
    rng = np.random.default_rng(7)
    acts = R.random_playouts(n, seed=11, stride=80)
    length = (acts != 255).sum(axis=1)
    kind = rng.integers(0, 3, n)
    cut = rng.integers(0, length + 1)
    col = np.arange(80)[None, :]
    acts[(kind == 1)[:, None] & (col >= cut[:, None])] = 255
    hit = np.flatnonzero(kind == 2)
    acts[hit, rng.integers(0, length[hit])] = rng.integers(0, 256, len(hit)).astype(np.uint8)
    winner = rng.integers(-1, 2, n).astype(np.int8)
    head = np.full((n, 16), 255, np.uint8)
    head[:, :4] = acts[:, :4]
    start = R.replay_cpu_raw(head, None, None, None, 16, 0)
    ok = (start["n_rows"] == 4) & (start["final_colour"] == 1)  # four placements, no stop
    rest = np.full((n, 80), 255, np.uint8)
    rest[:, :76] = acts[:, 4:]
    return {"acts": acts, "winner": winner, "rest": rest[ok], "own0": start["final_own"][ok],
            "opp0": start["final_opp"][ok], "winner0": winner[ok]}


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("start", [False, True])
def test_random_playouts_bit_identical(mixed, stride, flags, start):
    if start:
        acts, own0, opp0, w = mixed["rest"], mixed["own0"], mixed["opp0"], mixed["winner0"]
        assert len(acts) > 3000
    else:
        acts, own0, opp0, w = mixed["acts"], None, None, mixed["winner"]
        assert len(acts) == 4099
    acts = np.ascontiguousarray(acts[:, :stride])  # stride 64 cuts the longest games short
    cpu, gpu = both(acts, own0, opp0, w, max_rows=stride, flags=flags)
    assert_identical(cpu, gpu)
    # the mix is what it says: every status but overflow
    seen = set(np.unique(cpu["status"]))
    assert {nat.AZ_REC_TERMINAL, nat.AZ_REC_UNFINISHED, nat.AZ_REC_ILLEGAL} <= seen
    # derived winners and a row limit the games overflow
    cpu, gpu = both(acts, own0, opp0, None, max_rows=40, flags=flags)
    assert_identical(cpu, gpu)
    assert (cpu["status"] == nat.AZ_REC_OVERFLOW).any()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_small_batches(gold, n):
    acts = np.concatenate([gold["free_acts"], gold["trunc_acts"]])[:n]
    cpu, gpu = both(acts)
    assert_identical(cpu, gpu)
    assert cpu["n_rows"][0] == gold["free_len"][0]


def test_empty_batch_and_argument_errors():
    out = R.replay_gpu_raw(torch.zeros((0, 64), dtype=torch.uint8, device="cuda"), None, None,
                           None, 64, 0)
    assert out["n_rows"].shape == (0,)
    a = torch.full((2, 64), 255, dtype=torch.uint8, device="cuda")
    keep = R.replay_gpu_raw(a, None, None, None, 64, 0)
    bufs = [nat.ptr(keep[k]) for k in R._ORDER]
    call = nat.lib.oth_records_gpu
    assert call(None, 64, None, None, None, 2, 64, 0, *bufs, None) == nat.AZ_ERR_ARG
    assert call(nat.ptr(a), 48 + 8, None, None, None, 2, 64, 0, *bufs, None) == nat.AZ_ERR_ARG
    assert call(nat.ptr(a), 64, None, None, None, 2, 129, 0, *bufs, None) == nat.AZ_ERR_ARG
    assert call(ctypes.c_void_p(a.data_ptr() + 8), 64, None, None, None, 1, 64, 0, *bufs,
                None) == nat.AZ_ERR_ARG
    torch.cuda.synchronize()


# ---- majority vote -------------------------------------------------------------------------

def assert_vote_equals_mirror(own, opp, act, z):
    want = R.vote_numpy(own, opp, act, z)
    got = R.vote_gpu_tensors(dev(own), dev(opp), dev(act), dev(z))
    torch.cuda.synchronize()
    got = [g.cpu().numpy() for g in got]
    got[0], got[1] = got[0].view(np.uint64), got[1].view(np.uint64)
    assert len(got) == len(want) == 5
    for g, w, name in zip(got, want, ("own", "opp", "act", "z", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert (g == w).all(), name
    return want


def test_vote_fixture_rows(gold):
    own, opp, act, z, count = assert_vote_equals_mirror(
        gold["vote_in_own"], gold["vote_in_opp"], gold["vote_in_act"], gold["vote_in_z"])
    # and so the reference's output, order included
    assert (own == gold["vote_out_own"]).all() and (opp == gold["vote_out_opp"]).all()
    assert (act == gold["vote_out_act"]).all() and (z == gold["vote_out_z"]).all()


def test_vote_one_huge_group_with_a_tie(gold):
    rng = np.random.default_rng(3)
    rows, prow = gold["free_row_ply"] >= 4, gold["pass_row_ply"] >= 4  # no initial position
    own = np.concatenate([gold["free_row_own"][rows], gold["pass_row_own"][prow]])[:15000]
    opp = np.concatenate([gold["free_row_opp"][rows], gold["pass_row_opp"][prow]])[:15000]
    m = len(own)
    assert m >= 4000
    own, opp = np.resize(own, 15000), np.resize(opp, 15000)  # repeats: groups of 3 or 4
    act = rng.integers(0, 65, 15000).astype(np.uint8)
    z = rng.integers(-1, 2, 15000).astype(np.int8)
    # 5,000 copies of the initial position: two actions and two outcomes tie at 2,000
    init_act = np.repeat([19, 26, 37, 44], [2000, 2000, 600, 400]).astype(np.uint8)
    init_z = np.repeat([1, -1, 0], [2000, 2000, 1000]).astype(np.int8)
    own = np.concatenate([own, np.full(5000, R.INIT_OWN, np.uint64)])
    opp = np.concatenate([opp, np.full(5000, R.INIT_OPP, np.uint64)])
    act, z = np.concatenate([act, rng.permutation(init_act)]), np.concatenate([z, rng.permutation(init_z)])
    order = rng.permutation(20000)
    own, opp, act, z = own[order], opp[order], act[order], z[order]
    res = assert_vote_equals_mirror(own, opp, act, z)
    g = np.flatnonzero((res[0] == R.INIT_OWN) & (res[1] == R.INIT_OPP))
    assert len(g) == 1 and res[4][g[0]] == 5000
    init = (own == R.INIT_OWN) & (opp == R.INIT_OPP)
    first = {v: int(np.flatnonzero(init & (act == v))[0]) for v in (19, 26)}
    assert res[2][g[0]] == min(first, key=first.get)
    firstz = {v: int(np.flatnonzero(init & (z == v))[0]) for v in (1, -1)}
    assert res[3][g[0]] == min(firstz, key=firstz.get)
    assert res[4].sum() == 20000


def test_vote_all_unique_and_single_row(gold):
    pair = np.unique(np.stack([gold["free_row_own"], gold["free_row_opp"]], axis=1), axis=0)
    rng = np.random.default_rng(5)
    pair = pair[rng.permutation(len(pair))]
    own, opp = np.ascontiguousarray(pair[:, 0]), np.ascontiguousarray(pair[:, 1])
    act = rng.integers(0, 65, len(own)).astype(np.uint8)
    z = rng.integers(-1, 2, len(own)).astype(np.int8)
    res = assert_vote_equals_mirror(own, opp, act, z)
    assert (res[0] == own).all() and (res[2] == act).all() and (res[4] == 1).all()
    res = assert_vote_equals_mirror(own[:1], opp[:1], act[:1], z[:1])
    assert len(res[0]) == 1
    assert all(len(x) == 0 for x in R.vote_gpu_tensors(dev(own[:0]), dev(opp[:0]), dev(act[:0]),
                                                       dev(z[:0])))


def test_vote_workspace_query(gold):
    own, opp = dev(gold["vote_in_own"]), dev(gold["vote_in_opp"])
    act, z = dev(gold["vote_in_act"]), dev(gold["vote_in_z"])
    n = own.numel()
    outs = [torch.empty(n, dtype=dt, device="cuda")
            for dt in (torch.int64, torch.int64, torch.uint8, torch.int8, torch.int32)]
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = [nat.ptr(own), nat.ptr(opp), nat.ptr(act), nat.ptr(z), n, *[nat.ptr(o) for o in outs],
            nat.ptr(n_out)]
    need = ctypes.c_size_t(0)
    assert nat.lib.az_records_vote_gpu(*args, None, ctypes.byref(need), None) == nat.AZ_OK
    assert need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    short = ctypes.c_size_t(need.value - 1)
    assert nat.lib.az_records_vote_gpu(*args, nat.ptr(ws), ctypes.byref(short),
                                       nat.stream_ptr()) == nat.AZ_ERR_ARG
    exact = ctypes.c_size_t(need.value)
    assert nat.lib.az_records_vote_gpu(*args, nat.ptr(ws), ctypes.byref(exact),
                                       nat.stream_ptr()) == nat.AZ_OK
    torch.cuda.synchronize()
    assert int(n_out.item()) == len(gold["vote_out_own"])
    assert (outs[2][:int(n_out.item())].cpu().numpy() == gold["vote_out_act"]).all()


def test_dedup_mean_on_device_equals_host(gold):
    rows = (gold["vote_in_own"], gold["vote_in_opp"], gold["vote_in_act"], gold["vote_in_z"])
    want = R.dedup(*rows, how="mean", device="cpu")
    got = R.dedup(*rows, how="mean", device="cuda")
    assert (got["own"] == want["own"]).all() and (got["count"] == want["count"]).all()
    # the device renormalises the same float32 shares k / size by their float32 sum: 12
    # additions on the longest path of NumPy's pairwise sum of 65 entries (8 per partial, 3 to
    # join the partials, the tail) and one division, half an ulp of 1 each, on entries <= 1
    assert np.abs(got["pi"] - want["pi"]).max() <= 6.5 * np.finfo(np.float32).eps
    assert (got["z"] == want["z"]).all()


# ---- end to end ----------------------------------------------------------------------------

def test_records_to_supervised_fit(gold):
    import train_gpu
    from Models import AlphaZeroNet

    torch.manual_seed(0)
    acts, winner = dev(gold["free_acts"]), dev(gold["free_winner"])
    own, opp, act, z, ply, game, report = R.replay(acts, winner=winner)
    assert own.is_cuda and own.dtype == torch.int64 and len(own) == int(gold["free_len"].sum())
    assert (own.cpu().numpy().view(np.uint64) == gold["free_row_own"]).all()
    assert (game.cpu().numpy() == gold["free_row_game"]).all()
    assert not bool(report["winner_mismatch"].any()) and bool(report["kept"].all())
    rows = R.dedup(own, opp, act, z, how="vote")
    assert rows["own"].is_cuda and int(rows["count"].sum()) == len(own)
    loader = train_gpu.DeviceReplayLoader.from_bitboards(
        rows["own"], rows["opp"], rows["act"], rows["z"], batch_size=256, seed=1)
    seen = 0
    for state, pi, v in loader:
        b = state.shape[0]
        assert state.shape == (b, 1, 8, 8) and pi.shape == (b, 65) and v.shape == (b, 1)
        assert state.dtype == pi.dtype == v.dtype == torch.float32 and state.is_cuda
        assert bool(((state == 0) | (state == 1) | (state == -1)).all())
        assert bool((pi.sum(dim=1) == 1).all()) and bool(((pi == 0) | (pi == 1)).all())
        assert bool((v.abs() <= 1).all())
        seen += b
    assert seen == len(rows["own"]) and len(loader) == -(-seen // 256)
    # 30 optimiser steps over the same 64 rows lower the loss the net started with
    sub = [rows[k][:64] for k in ("own", "opp", "act", "z")]
    fit = train_gpu.DeviceReplayLoader.from_bitboards(*sub, batch_size=64, seed=2)
    held = train_gpu.DeviceReplayLoader.from_bitboards(*sub, batch_size=64, shuffle=False,
                                                       augment=False)
    net = AlphaZeroNet(8, 65, 2, 16).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=3e-3)
    before = train_gpu.supervised_eval(net, held)
    for _ in range(30):
        assert len(fit) == 1
        loss = train_gpu.supervised_epoch(net, opt, fit)
        assert np.isfinite(loss)
    after = train_gpu.supervised_eval(net, held)
    print("supervised_eval before", before, "after", after)
    assert after[0] < before[0]
    assert 0.0 <= after[3] <= 1.0 and len(after) == 4
