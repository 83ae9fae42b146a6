"""Record tests/golden/source_bits.json: SHA-256 digests of what the source-estimate kernels write.

The four-term kernels (csrc/source_fit.hip), the six-term kernels (csrc/source_aniso.hip) and the stop scan share their record
reader, contributions, Cholesky and summary pieces (csrc/source_core.h, csrc/source_solve.h).  How that code is laid out may change;
what the kernels compute must not.  tests/test_gpu_source_bits.py compares every output buffer of the cases below, whole, with the
digests recorded here -- by the build BEFORE such a change, on the GPU:

    python tools/gen_golden_source_bits.py [OUT]    # at the parent commit of the change; OUT defaults to the golden file

Only uavppo.ops calls are used, and numpy for the inputs (tests/_source_*_cases.py; eval_track.reduce_chunk for the `ended` between
two pieces): nothing that restates the kernels takes part.  "iso" is uav_source_moments / _solve / _summary, "aniso" the *6 entry points.

moments  (n, k, D) in (1, 1, 6), (65, 65, 6), (5, 250, 8) from episodes / episodes6, with the turbulence channel and with a constant
         background, in one chunk and (k > 1) cut in two at k // 2 with `ended` from the reduce between: the state.
solve    on each of those states, and on the states of the every-status cases (48 envs of the twelve kinds at k = 64 / 63), at the
         default cfg and at the model's least min_samples with min_pivot 1e-3: est (all of it: peak and strength too) and status.
summary  n in (1, 257) from estimates / estimates6, with and without the truth, with and without loc_err: sums and loc_err.
stop     uav_source_stop_scan with mark 0 and 1 on the three case sets of the smallest of _source_stop_cases.SHAPES, of SPLIT_SHAPES[0]
         cut at 63, and on placed_hits (a hit in lane 0, in lane 63, in a chunk's first record, on a done record; idle envs): per
         piece the state, first_hit, mu_steps, status_steps, the flags and `active`.
"""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "uav-wrf-les-ppo-lstm_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
PATH = os.path.join(ROOT, "tests", "golden", "source_bits.json")
MOMENT_SHAPES = ((1, 1, 6), (65, 65, 6), (5, 250, 8))
STATUS_SHAPES = {"iso": (48, 64, 6), "aniso": (48, 63, 6)}
SUMMARY_N = (1, 257)
TKE = {"tke": {}, "background": dict(use_tke=False, background=2.9, floor=20.0)}
SOLVE_CFGS = {"iso": ({}, dict(min_samples=4, min_pivot=1e-3)), "aniso": (dict(min_samples=8), dict(min_samples=6, min_pivot=1e-3))}
STOP_SPLIT = 63
NAN = float("nan")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _model(model):
    """(episodes, estimates, moments, solve, est width) of a model"""
    from uavppo import ops
    import _source_aniso_cases as ca
    import _source_fit_cases as cf
    if model == "iso":
        return cf.episodes, cf.estimates, ops.source_moments, ops.source_solve, ops.SRC_EST_N
    return ca.episodes6, ca.estimates6, ops.source_moments6, ops.source_solve6, ops.SRC6_EST_N


def run_moments(model, n, k, D, kw, split):
    """the state after the chunk (split: in two pieces, the second's `ended` from eval_track.reduce_chunk over the first)"""
    from uavppo import eval_track as et, ops
    episodes, _, moments, _, _ = _model(model)
    ep = episodes(n, k, D)
    st, cfg = _dev(ep["state"]), ops.source_fit_cfg(**dict(SOLVE_CFGS[model][0], **kw))
    eps = (np.zeros(n, np.int32), ep["ended"].copy(), np.zeros((n, 2)))
    cuts = [0, k // 2, k] if split else [0, k]
    for a, b in zip(cuts[:-1], cuts[1:]):
        f, o, p = ep["flags"][:, a:b], ep["obs"][:, a:b], ep["pos"][:, a:b]
        moments({"flags": _dev(f), "obs": _dev(o), "pos": _dev(p)}, cfg, st, _dev(eps[1]))
        eps = et.reduce_chunk(f, o, p, a, *eps)
    torch.cuda.synchronize()
    return st


def run_solve(model, state):
    from uavppo import ops
    _, _, _, solve, est_n = _model(model)
    out = {}
    for j, kw in enumerate(SOLVE_CFGS[model]):
        est = torch.full((state.shape[0], est_n), -7.0, dtype=torch.float64, device=DEV)
        status = torch.full((state.shape[0],), 99, dtype=torch.uint8, device=DEV)
        solve(state, ops.source_fit_cfg(**kw), est, status)
        out["cfg%d.est" % j], out["cfg%d.status" % j] = est, status
    torch.cuda.synchronize()
    return out


def _moments_case(model, n, k, D, tke, split):
    def case():
        st = run_moments(model, n, k, D, TKE[tke], split)
        return dict(run_solve(model, st), state=st)
    return case


def _summary_case(model, n):
    def case():
        from uavppo import ops
        got = _model(model)[1](n)
        est, status, src = (_dev(a) for a in got[:3])
        out = {}
        for truth in (True, False):
            for per_env in (True, False):
                sums = torch.full((ops.SRC_SUM_N if model == "iso" else ops.SRC6_SUM_N,), -7.0, dtype=torch.float64, device=DEV)
                loc = torch.full((n,), -7.0, dtype=torch.float64, device=DEV) if per_env else None
                if model == "iso":
                    ops.source_summary(est, status, src, 500.0 / 16.0 if truth else NAN, 100.0 if truth else NAN, 5.0, sums, loc_err=loc)
                else:
                    ops.source_summary6(est, status, src, _dev(got[3]) if truth else None, 5.0, sums, loc_err=loc)
                tag = ("truth" if truth else "notruth") + ("-loc" if per_env else "-noloc")
                out[tag + ".sums"] = sums
                if per_env:
                    out[tag + ".loc_err"] = loc
        torch.cuda.synchronize()
        return out
    return case


def device_scan(mark):
    """uav_source_stop_scan behind source_stop.stop_scan_chunk's signature, for _source_stop_cases.drive"""
    def scan(flags, obs, pos, t0, state, ended, fit_cfg, stop_cfg):
        from uavppo import ops
        n, k = flags.shape
        recs = {"flags": _dev(flags), "obs": _dev(obs), "pos": _dev(pos)}
        out = {"state": _dev(np.array(state)), "first_hit": torch.full((n,), -9, dtype=torch.int32, device=DEV), "flags": recs["flags"],
               "active": torch.ones(n, dtype=torch.uint8, device=DEV), "mu_steps": torch.full((n, k, 2), -7.0, dtype=torch.float64, device=DEV),
               "status_steps": torch.full((n, k), 99, dtype=torch.uint8, device=DEV)}
        ops.source_stop_scan(recs, t0, ops.source_fit_cfg(**fit_cfg), ops.source_stop_cfg(**stop_cfg), out["state"], out["first_hit"],
                             _dev(np.array(ended)), out["active"], out["mu_steps"], out["status_steps"], mark=mark)
        return {key: v.cpu().numpy() for key, v in out.items()}
    return scan


@functools.lru_cache(None)
def stop_sets():
    """name -> (records, fit cfg keywords, stop cfg keywords, cuts)"""
    import _source_stop_cases as cs
    sets = {}
    for shape, cut in ((min(cs.SHAPES, key=lambda s: s[0] * s[1]), None), (cs.SPLIT_SHAPES[0], STOP_SPLIT)):
        n, k = shape[:2]
        for name, ep, kw in cs.case_sets(*shape):
            sets["n%d-k%d-%s" % (n, k, name.replace(",", "").replace(" ", "_"))] = (ep, kw, {}, [0, k] if cut is None else [0, cut, k])
    for name, ep, kw, stop, split, _ in cs.placed_hits():
        k = ep["flags"].shape[1]
        sets["placed-" + name.replace(",", "").replace("'", "").replace(" ", "_")] = (ep, kw, stop, [0, k] if split is None else [0, split, k])
    return sets


def _stop_case(name, mark):
    def case():
        import _source_stop_cases as cs
        from uavppo import source_fit as sf, source_stop as ss
        ep, kw, stop, cuts = stop_sets()[name]
        _, outs = cs.drive(ss, ep, sf.check_source_fit(**kw), ss.check_source_stop(**stop), cuts, scan=device_scan(mark))
        return {"piece%d.%s" % (j, key): torch.from_numpy(np.ascontiguousarray(o[key])) for j, o in enumerate(outs)
                for key in ("state", "first_hit", "mu_steps", "status_steps", "flags", "active")}
    return case


def cases():
    """name -> callable() -> {buffer name: tensor}"""
    c = {}
    for model in ("iso", "aniso"):
        for n, k, D in MOMENT_SHAPES + (STATUS_SHAPES[model],):
            for tke in TKE:
                for split in ((False, True) if k > 1 else (False,)):
                    c["moments-%s-n%d-k%d-D%d-%s-%s" % (model, n, k, D, tke, "split" if split else "whole")] = _moments_case(model, n, k, D, tke, split)
        for n in SUMMARY_N:
            c["summary-%s-n%d" % (model, n)] = _summary_case(model, n)
    for name in stop_sets():
        for mark in (0, 1):
            c["stop-%s-mark%d" % (name, mark)] = _stop_case(name, mark)
    return c


def run_case(name):
    return {k: _sha(v) for k, v in cases()[name]().items()}


def main():
    out = {}
    for name in cases():
        out[name] = run_case(name)
        assert run_case(name) == out[name], f"{name}: two runs differ"
        print(f"{name}: {len(out[name])} buffers")
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
