"""uav_source_stop_scan (csrc/source_fit.hip) against the numpy statement of uavppo/source_stop.py on synthetic records
(tests/_source_stop_cases.py; their margins are asserted in tests/test_source_stop_host.py).  With a rule that cannot fire the
scan's accumulators are the statement's (count, centre and A bit for bit, g within the rounding of its sum) and its per-record
statuses and estimates the statement's; with the rule on, its decisions are stop_rule on its own estimates exactly and the
statement's for every env.  evaluate() and the trainer are in tests/test_gpu_source_stop_eval.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _source_stop_cases import SHAPES, SPLIT_SHAPES, SPLITS, case_sets, drive, placed_hits, start_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = [0, 1, 2] + list(range(3, 13))                         # count, centre, A
G = [13, 14, 15, 16]


@pytest.fixture(scope="module")
def ops():
    from uavppo import ops as o
    return o


@pytest.fixture(scope="module")
def sf():
    from uavppo import source_fit
    return source_fit


@pytest.fixture(scope="module")
def ss():
    from uavppo import source_stop
    return source_stop


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_scan(ops, per_record=True):
    """uav_source_stop_scan behind stop_scan_chunk's signature (for _source_stop_cases.drive): numpy in, numpy out, and `active`
    (all ones going in)."""
    def scan(flags, obs, pos, t0, state, ended, fit_cfg, stop_cfg):
        n, k = flags.shape
        recs = {"flags": dev(flags), "obs": dev(obs), "pos": dev(pos)}
        st, first = dev(np.array(state)), torch.full((n,), -9, dtype=torch.int32, device=DEV)
        active = torch.ones(n, dtype=torch.uint8, device=DEV)
        mu = torch.full((n, k, 2), -7.0, dtype=torch.float64, device=DEV) if per_record else None
        status = torch.full((n, k), 99, dtype=torch.uint8, device=DEV) if per_record else None
        ops.source_stop_scan(recs, t0, ops.source_fit_cfg(**fit_cfg), ops.source_stop_cfg(**stop_cfg), st, first, dev(np.array(ended)),
                             active, mu, status, mark=True)
        return {"state": st.cpu().numpy(), "first_hit": first.cpu().numpy(), "flags": recs["flags"].cpu().numpy(),
                "active": active.cpu().numpy(), "mu_steps": None if mu is None else mu.cpu().numpy(),
                "status_steps": None if status is None else status.cpu().numpy()}
    return scan


def _g_bound(sf, flags, obs, pos, ended, state, **kw):
    """(n_used + 4) 2^-52 sum |w phi_j ln b| per env and j over one piece's used records: the bound of the moments test"""
    used, b, cell = sf.used_records(flags, obs, pos, ended, **kw)
    p = (cell[:, :, 0] - state[:, 1:2]) / 32.0
    q = (cell[:, :, 1] - state[:, 2:3]) / 32.0
    bu = np.where(used, b, 1.0)
    t = np.where(used, bu * bu * np.abs(np.log(bu)), 0.0)
    phi = np.stack([np.ones_like(p), np.abs(p), np.abs(q), p * p + q * q], 2)
    return (used.sum(1) + 4.0)[:, None] * 2.0 ** -52 * (t[:, :, None] * phi).sum(1)


def _no_hit(ops, sf, ss, ep, kw, cuts):
    """One case set with a rule that cannot fire, over the pieces `cuts`; returns the largest |mu - statement's| on FITTED records."""
    fit_cfg, cannot = sf.check_source_fit(**kw), ss.check_source_stop(patience=1 << 30)
    want_st, want = drive(ss, ep, fit_cfg, cannot, cuts)
    got_st, got = drive(ss, ep, fit_cfg, cannot, cuts, scan=device_scan(ops))
    bound, worst = 0.0, 0.0
    for w, g in zip(want, got):
        a, b = w["t0"], w["t0"] + w["flags"].shape[1]
        f, o, p = ep["flags"][:, a:b], ep["obs"][:, a:b], ep["pos"][:, a:b]
        only = {key: fit_cfg[key] for key in ("use_tke", "background", "floor")}
        bound = bound + _g_bound(sf, f, o, p, (w["ended"] != 0).astype(np.uint8), w["state"], **only)
        assert np.array_equal(bits64(g["state"][:, EXACT]), bits64(w["state"][:, EXACT]))
        assert (np.abs(g["state"][:, G] - w["state"][:, G]) <= bound).all()
        assert np.array_equal(g["status_steps"], w["status_steps"])
        fit = w["status_steps"] == 0
        assert np.isnan(g["mu_steps"][~fit]).all() and not np.isnan(g["mu_steps"][fit]).any()
        if fit.any():
            worst = max(worst, float(np.abs(g["mu_steps"][fit] - w["mu_steps"][fit]).max()))
        assert (g["first_hit"] == -1).all() and np.array_equal(g["flags"], f) and (g["active"] == 1).all()
        assert not np.isnan(g["state"]).any()
        gone = w["ended"] != 0
        assert np.array_equal(bits64(g["state"][gone]), bits64(w["start"][gone]))          # untouched to the bit
    assert worst <= 1e-6
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-k%d-D%d" % s[:3])
def test_a_scan_that_cannot_fire_is_the_statement(ops, sf, ss, shape):
    n, k, D, seed = shape
    worst = max(_no_hit(ops, sf, ss, ep, kw, [0, k]) for name, ep, kw in case_sets(n, k, D, seed))
    print(f"n={n} k={k} D={D}: max |mu - statement| on FITTED records {worst:.3e} cells")


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "n%d-k%d-D%d" % s[:3])
def test_two_chunk_splits_that_cannot_fire_are_the_statement(ops, sf, ss, shape):
    n, k, D, seed = shape
    worst = max(_no_hit(ops, sf, ss, ep, kw, [0, s, k]) for s in SPLITS for name, ep, kw in case_sets(n, k, D, seed))
    print(f"n={n} k={k} D={D}, splits {SPLITS}: max |mu - statement| on FITTED records {worst:.3e} cells")


def _rule_on(ops, sf, ss, ep, kw, skw, cuts):
    """One case set with the rule on: the device's decisions are stop_rule on its own estimates exactly, and the statement's."""
    fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop(**skw)
    want_st, want = drive(ss, ep, fit_cfg, stop_cfg, cuts)
    got_st, got = drive(ss, ep, fit_cfg, stop_cfg, cuts, scan=device_scan(ops))
    for w, g in zip(want, got):
        a, b = w["t0"], w["t0"] + w["flags"].shape[1]
        f, p = ep["flags"][:, a:b], ep["pos"][:, a:b]
        idle = (g["ended"] != 0) | (g["start"][:, ss.HIT_STEP] > 0)
        first, rs = ss.stop_rule(g["mu_steps"], g["status_steps"], p, a, g["start"][:, ss.RULE], stop_cfg)
        assert np.array_equal(g["first_hit"], first)
        assert np.array_equal(bits64(g["state"][~idle][:, ss.RULE]), bits64(rs[~idle]))
        assert np.array_equal(g["flags"], ss.mark_flags(f, first))
        assert np.array_equal(g["first_hit"], w["first_hit"])                              # licensed by the margins of the inputs
        assert np.array_equal(g["flags"], w["flags"]) and np.array_equal(g["status_steps"], w["status_steps"])
        assert np.array_equal(g["active"], (g["first_hit"] < 0).astype(np.uint8))          # cleared exactly at the hits
        assert (g["first_hit"][idle] == -1).all()
        assert np.array_equal(bits64(g["state"][idle]), bits64(g["start"][idle])) and np.array_equal(g["flags"][idle], f[idle])
        assert (g["status_steps"][idle] == 255).all() and np.isnan(g["mu_steps"][idle]).all()
        assert not np.isnan(g["state"]).any()
        assert np.array_equal(bits64(g["state"][:, EXACT]), bits64(w["state"][:, EXACT]))
        hit = g["first_hit"] >= 0
        # the estimate at the hit: mu within the project's 1e-6 cells; sigma, peak and strength within 1e-6 relative (that
        # tolerance against a cell scale of 1)
        assert (np.abs(g["state"][hit, ss.EST:ss.EST + 2] - w["state"][hit, ss.EST:ss.EST + 2]) <= 1e-6).all()
        assert (np.abs(g["state"][hit, ss.EST + 2:] - w["state"][hit, ss.EST + 2:]) <= 1e-6 * np.abs(w["state"][hit, ss.EST + 2:])).all()
    return got_st, got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-k%d-D%d" % s[:3])
def test_the_rule_decides_as_stop_rule_and_as_the_statement(ops, sf, ss, shape):
    n, k, D, seed = shape
    hits = 0
    for name, ep, kw in case_sets(n, k, D, seed):
        st, outs = _rule_on(ops, sf, ss, ep, kw, {}, [0, k])
        hits += int((outs[0]["first_hit"] >= 0).sum())
        # the same records again behind the hits: envs that come in already hit are untouched to the bit
        fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop()
        again = device_scan(ops)(outs[0]["flags"], ep["obs"], ep["pos"], k, st, np.zeros(n, np.uint8), fit_cfg, stop_cfg)
        was = st[:, ss.HIT_STEP] > 0
        assert (again["first_hit"][was] == -1).all() and np.array_equal(bits64(again["state"][was]), bits64(st[was]))
        assert np.array_equal(again["flags"][was], outs[0]["flags"][was]) and (again["active"][was] == 1).all()
    if k >= 63 and n >= 5:
        assert hits > n


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "n%d-k%d-D%d" % s[:3])
def test_the_rule_over_two_chunk_splits(ops, sf, ss, shape):
    n, k, D, seed = shape
    for s in SPLITS:
        for name, ep, kw in case_sets(n, k, D, seed):
            _rule_on(ops, sf, ss, ep, kw, {}, [0, s, k])


def test_placed_hits_and_the_outputs_that_may_be_left_out(ops, sf, ss):
    """A hit on lane 0 and on lane 63 of a block, on a chunk's first record with the run carried in, on the record that is also
    done; near and min_steps; NULL mu_steps / status_steps give the same state, first_hit and flags; mark = 0 writes
    neither flags nor active."""
    for name, ep, kw, skw, split, at in placed_hits():
        k = ep["flags"].shape[1]
        st, outs = _rule_on(ops, sf, ss, ep, kw, skw, [0, k] if split is None else [0, split, k])
        assert ((st[:, ss.HIT_STEP] == at + 1).sum() >= 5) if at is not None else (st[:, ss.HIT_STEP] > 0).sum() >= 5, name
    name, ep, kw, skw, split, at = placed_hits()[0]
    n, k = ep["flags"].shape
    fit_cfg, stop_cfg = sf.check_source_fit(**kw), ss.check_source_stop(**skw)
    full = device_scan(ops)(ep["flags"], ep["obs"], ep["pos"], 0, start_state(ep), ep["ended"], fit_cfg, stop_cfg)
    bare = device_scan(ops, per_record=False)(ep["flags"], ep["obs"], ep["pos"], 0, start_state(ep), ep["ended"], fit_cfg, stop_cfg)
    for key in ("state", "first_hit", "flags", "active"):
        assert np.array_equal(full[key], bare[key]), key
    recs = {"flags": dev(ep["flags"]), "obs": dev(ep["obs"]), "pos": dev(ep["pos"])}
    stop = ss.SourceStop(n, DEV, fit_cfg=kw, **skw)
    stop.state.fill_(3.0)
    stop.restart()
    active = torch.ones(n, dtype=torch.uint8, device=DEV)
    first = stop.scan(recs, 0, None, active, mark=False).cpu().numpy()                     # ended may be NULL; no mark: active stays
    assert (first >= 0).sum() >= 5
    assert np.array_equal(first, full["first_hit"]) and np.array_equal(recs["flags"].cpu().numpy(), ep["flags"])
    assert np.array_equal(bits64(stop.state.cpu().numpy()), bits64(full["state"])) and (active == 1).all()
    assert np.array_equal(stop.stop_steps().cpu().numpy(), full["state"][:, ss.HIT_STEP].astype(np.int64))


def test_the_entry_point_refuses_with_a_reason(ops):
    from uavppo import _lib
    lib, h = _lib.lib(), ops.Context.get(torch.device(DEV)).handle
    a = torch.zeros(4096, dtype=torch.float64, device=DEV)
    p = C.c_void_p(a.data_ptr())
    odd = C.c_void_p(a.data_ptr() + 4)
    nan, inf = float("nan"), float("inf")
    g, s = C.byref(ops.source_fit_cfg()), C.byref(ops.source_stop_cfg())

    def cfg(**kw):
        return C.byref(ops.source_fit_cfg(**kw))

    def stop(**kw):
        return C.byref(ops.source_stop_cfg(**kw))

    # (flags, obs, pos, n, k, D, t0, cfg, stop, ended, active, state, first_hit, mu_steps, status_steps, mark)
    def args(flags=p, obs=p, pos=p, n=1, k=1, D=6, t0=0, c=g, st=s, state=p, first=p):
        return (flags, obs, pos, n, k, D, t0, c, st, None, None, state, first, None, None, 1)

    for ar, what in ((args(flags=None), b"NULL"), (args(obs=None), b"NULL"), (args(pos=None), b"NULL"), (args(state=None), b"NULL"),
                     (args(first=None), b"NULL"), (args(c=None), b"NULL cfg"), (args(st=None), b"NULL stop cfg"),
                     (args(n=0), b"at least 1"), (args(k=0), b"at least 1"), (args(D=3), b"at least 4"),
                     (args(D=2, c=cfg(use_tke=False)), b"at least 3"), (args(n=1 << 12, k=1 << 12, D=128), b"2^31"),
                     (args(t0=-1), b"t0"), (args(t0=(1 << 31) - 1), b"t0"), (args(pos=odd), b"aligned"),
                     (args(c=cfg(min_samples=3)), b"min_samples"), (args(c=cfg(floor=nan)), b"floor"),
                     (args(c=cfg(background=inf)), b"background"), (args(c=cfg(min_pivot=0.0)), b"min_pivot"),
                     (args(st=stop(settle_tol=-1.0)), b"settle_tol"), (args(st=stop(settle_tol=nan)), b"settle_tol"),
                     (args(st=stop(settle_tol=inf)), b"settle_tol"), (args(st=stop(near=nan)), b"near"),
                     (args(st=stop(near=-0.5)), b"near"), (args(st=stop(patience=0)), b"patience"),
                     (args(st=stop(min_steps=-1)), b"min_steps")):
        assert lib.uav_source_stop_scan(h, *ar, None) == 2 and what in lib.uav_last_error(), (what, lib.uav_last_error())
    st = C.c_void_p(a.data_ptr() + 8 * 1024)
    first = C.c_void_p(a.data_ptr() + 8 * 2048)
    ok = (p, p, p, 1, 1, 3, 0, cfg(use_tke=False), stop(near=inf), None, None, st, first, None, None, 0)
    assert lib.uav_source_stop_scan(h, *ok, None) == 0                                     # D = 3 without obs[3]; near = inf
    torch.cuda.synchronize()
