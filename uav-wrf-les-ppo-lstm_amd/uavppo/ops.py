"""Tensor-level wrappers over the C ABI: shape/dtype/device checks on the host, then one call
into libuavppo.so on torch's current HIP stream.  PyTorch only supplies device memory and
streams here; every number is produced by the hand-written HIP kernels."""
from __future__ import annotations

import contextlib
import ctypes as C
import types

import torch

from . import _lib
from ._lib import EnvCfg, check, lib

GAE_MODES = {"reference_exact": 0, "standard": 1, "inline_v10": 2}
WS_BYTES = 256 << 20


class Context:
    """One uav_ctx per device (opaque handle: CU count + scratch workspace)."""
    _per_device: dict = {}

    def __init__(self, device_index):
        if not torch.cuda.is_available():
            raise RuntimeError("uavppo needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                               "and there is no CPU fallback")
        h = C.c_void_p()
        check(lib().uav_create(C.byref(h), int(device_index), WS_BYTES), "uav_create")
        self.handle = h
        self.device = device_index
        # the mode uav_create started the handle in (UAV_LSTM_F32_MFMA / UAV_LSTM_BF16X6 in the environment, read there once)
        self.initial_arith = {0: "fp16x3", 1: "bf16x6", 2: "f32_mfma"}[int(lib().uav_get_lstm_arith(h))]

    @classmethod
    def get(cls, device=None):
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()
        if idx not in cls._per_device:
            cls._per_device[idx] = cls(idx)
        return cls._per_device[idx]


def _h(t):
    return Context.get(t.device).handle


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, dtype=None, shape=None, name="tensor"):
    """Device pointer of a checked tensor (None passes through as NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr())


F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8


class _KernelTimer:
    """Optional HIP-event bracket around named launches on torch's current stream (bench.py uses it
    to time the dominant kernel live inside the timed region).  Disabled = zero overhead."""

    CAP = 48      # brackets kept per name: HIP hands timing events out of a pool of ~1 k; the allocation that grows it stalls
                  # the host for ~30 ms (seen as one slow iteration around the 37th of a run that bracketed every launch)

    def __init__(self):
        self.names, self.events = (), {}

    def enable(self, names):
        self.names, self.events = tuple(names), {n: [] for n in names}

    def disable(self):
        self.names, self.events = (), {}

    def bracket(self, name):
        if name not in self.names or len(self.events[name]) >= self.CAP:
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.events[name].append((a, b))
        a.record()
        return b

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for n, ev in self.events.items():
            if ev:
                ms = [a.elapsed_time(b) for a, b in ev]
                out[n] = {"avg_ms": sum(ms) / len(ms), "n": len(ms)}
        return out


KERNEL_TIMER = _KernelTimer()


# ----------------------------------------------------------------------------- G1 / G2
def gae(rew, val, done, gamma, lam, mode="reference_exact", last_val=None, out=None):
    n, T = rew.shape
    adv = torch.empty_like(rew) if out is None else out
    check(lib().uav_gae(_h(rew), _p(rew, F32, (n, T), "rew"), _p(val, F32, (n, T), "val"),
                        _p(done, F32, (n, T), "done"), _p(last_val, F32, (n,), "last_val"), n, T,
                        float(gamma), float(lam), GAE_MODES[mode], _p(adv, F32, (n, T), "adv"), _stream()),
          "uav_gae")
    return adv


def adv_stats(adv, out=None):
    stats = torch.empty(3, dtype=F64, device=adv.device) if out is None else out
    check(lib().uav_adv_stats(_h(adv), _p(adv, F32, name="adv"), adv.numel(), _p(stats, F64, (3,), "stats3"),
                              _stream()), "uav_adv_stats")
    return stats


def adv_normalise(adv, val, stats3, adv_out=None, ret_out=None):
    adv_out = torch.empty_like(adv) if adv_out is None else adv_out
    ret_out = torch.empty_like(adv) if ret_out is None else ret_out
    if val.shape != adv.shape:
        raise RuntimeError("adv_normalise: val/adv shape mismatch")
    check(lib().uav_adv_normalise(_h(adv), _p(adv, F32, name="adv"), _p(val, F32, name="val"), adv.numel(),
                                  _p(stats3, F64, (3,), "stats3"), _p(adv_out, F32, adv.shape, "adv_out"),
                                  _p(ret_out, F32, adv.shape, "ret_out"), _stream()), "uav_adv_normalise")
    return adv_out, ret_out


def adv_normalise_inline(adv, val, stats3, adv_out=None, ret_out=None):
    """The inline update's normalisation (PPOV1.1/train_ppo1.0.py:86-89): ret_out = adv + val from the RAW advantage,
    adv_out = (adv - mean) / (std + 1e-8), unbiased std, no guard -- one sample gives NaN, as torch's .std() does."""
    adv_out = torch.empty_like(adv) if adv_out is None else adv_out
    ret_out = torch.empty_like(adv) if ret_out is None else ret_out
    if val.shape != adv.shape:
        raise RuntimeError("adv_normalise_inline: val/adv shape mismatch")
    check(lib().uav_adv_normalise_inline(_h(adv), _p(adv, F32, name="adv"), _p(val, F32, name="val"), adv.numel(),
                                         _p(stats3, F64, (3,), "stats3"), _p(adv_out, F32, adv.shape, "adv_out"),
                                         _p(ret_out, F32, adv.shape, "ret_out"), _stream()), "uav_adv_normalise_inline")
    return adv_out, ret_out


RETNORM_STATE_N = 4       # UAV_RETNORM_STATE_N: mean, M2, count, skipped


def return_stats(rew, done, carry, gamma, stats3=None, trace_out=None):
    """N1: the discounted return trace of rew / done f32 [n, T] in f64, continued from and into carry f64 [n] (in place);
    returns stats3 = {sum G, sum G^2, n T} (f64, device).  trace_out: f64 [n, T] to receive the traces, or None."""
    n, T = rew.shape
    stats3 = torch.empty(3, dtype=F64, device=rew.device) if stats3 is None else stats3
    check(lib().uav_return_stats(_h(rew), _p(rew, F32, (n, T), "rew"), _p(done, F32, (n, T), "done"), _p(carry, F64, (n,), "carry"),
                                 n, T, float(gamma), _p(stats3, F64, (3,), "stats3"), _p(trace_out, F64, (n, T), "trace_out"),
                                 _stream()), "uav_return_stats")
    return stats3


def return_norm_merge(state, stats3, eps=1e-8, scale=None):
    """N2: Chan's update of state f64 [4] = {mean, M2, count, skipped} (in place) by the batch sums stats3; returns
    scale f32 [1] = 1 / sqrt(M2 / count + eps) (1 without samples or variance).  No host sync."""
    scale = torch.empty(1, dtype=F32, device=state.device) if scale is None else scale
    check(lib().uav_return_norm_merge(_h(state), _p(state, F64, (RETNORM_STATE_N,), "state"), _p(stats3, F64, (3,), "stats3"),
                                      float(eps), _p(scale, F32, (1,), "scale"), _stream()), "uav_return_norm_merge")
    return scale


def reward_scale(rew, scale, clip=0.0, out=None):
    """N3: out = clamp(rew * scale[0], -clip, clip) in f32 (clip <= 0: no clamp); out may be rew."""
    out = torch.empty_like(rew) if out is None else out
    check(lib().uav_reward_scale(_h(rew), _p(rew, F32, name="rew"), rew.numel(), _p(scale, F32, (1,), "scale"), float(clip),
                                 _p(out, F32, rew.shape, "out"), _stream()), "uav_reward_scale")
    return out


def obs_norm_state_n(D):
    """UAV_OBSNORM_STATE_N(D): count, skipped, D means, D M2s."""
    return 2 + 2 * int(D)


def obs_stats(obs, stats=None):
    """O1: obs f32 [..., D] contiguous, or a 2-D view [rows, D] whose rows lie row_stride >= D floats apart -> stats f64
    [1 + 2 D] = {rows, channel sums, channel sums of squares} in the fixed order of obs_norm.batch_stats.  obs is not written."""
    if not obs.is_cuda or obs.dtype != F32 or obs.dim() < 2:
        raise RuntimeError("obs: expected a GPU f32 tensor [..., D]")
    D = obs.shape[-1]
    if obs.is_contiguous():
        rows, stride = obs.numel() // D, D
    elif obs.dim() == 2 and obs.stride(1) == 1 and obs.stride(0) >= D:
        rows, stride = obs.shape[0], obs.stride(0)
    else:
        raise RuntimeError("obs: expected a contiguous tensor, or a 2-D view with unit stride along the channels")
    stats = torch.empty(1 + 2 * D, dtype=F64, device=obs.device) if stats is None else stats
    check(lib().uav_obs_stats(_h(obs), C.c_void_p(obs.data_ptr()), rows, D, stride, _p(stats, F64, (1 + 2 * D,), "stats"), _stream()),
          "uav_obs_stats")
    return stats


def obs_norm_merge(state, stats, mask, eps, mu, inv_sigma):
    """O2: Chan's update per channel of state f64 [2 + 2 D] = {count, skipped, means, M2s} (in place) by the batch sums `stats`;
    writes mu, inv_sigma f32 [D].  mask: bit j set = channel j is normalised.  No host sync."""
    D = mu.numel()
    check(lib().uav_obs_norm_merge(_h(state), _p(state, F64, (obs_norm_state_n(D),), "state"), _p(stats, F64, (1 + 2 * D,), "stats"), D,
                                   int(mask), float(eps), _p(mu, F32, (D,), "mu"), _p(inv_sigma, F32, (D,), "inv_sigma"), _stream()),
          "uav_obs_norm_merge")
    return mu, inv_sigma


def obs_fold(w, b, mu, inv_sigma, w_eff, b_eff, pmax=None):
    """O3: the master first layer w [rows, D], b [rows] -> w_eff = w * inv_sigma, b_eff = b - w_eff . mu; pmax f32 [1] is raised
    to max |w_eff|, |b_eff|."""
    rows, D = w.shape
    check(lib().uav_obs_fold(_h(w), _p(w, F32, name="w"), _p(b, F32, (rows,), "b"), rows, D, _p(mu, F32, (D,), "mu"),
                             _p(inv_sigma, F32, (D,), "inv_sigma"), _p(w_eff, F32, (rows, D), "w_eff"), _p(b_eff, F32, (rows,), "b_eff"),
                             _p(pmax, F32, (1,), "pmax"), _stream()), "uav_obs_fold")
    return w_eff, b_eff


def obs_unfold_grad(dw, db, mu, inv_sigma):
    """O4, in place: dw [rows, D] <- (dw - db mu) * inv_sigma; db [rows] is only read."""
    rows, D = dw.shape
    check(lib().uav_obs_unfold_grad(_h(dw), _p(dw, F32, name="dw"), _p(db, F32, (rows,), "db"), rows, D, _p(mu, F32, (D,), "mu"),
                                    _p(inv_sigma, F32, (D,), "inv_sigma"), _stream()), "uav_obs_unfold_grad")
    return dw


def obs_unfold(w_eff, b_eff, mu, inv_sigma, w, b):
    """O5: the fold inverted: w = w_eff / inv_sigma, b = b_eff + w_eff . mu (w may be w_eff, b may be b_eff)."""
    rows, D = w_eff.shape
    check(lib().uav_obs_unfold(_h(w_eff), _p(w_eff, F32, name="w_eff"), _p(b_eff, F32, (rows,), "b_eff"), rows, D,
                               _p(mu, F32, (D,), "mu"), _p(inv_sigma, F32, (D,), "inv_sigma"), _p(w, F32, (rows, D), "w"),
                               _p(b, F32, (rows,), "b"), _stream()), "uav_obs_unfold")
    return w, b


def pack_success_bits(flags, cap, out=None):
    """flags u8 [..] -> u8 [4 + cap + 1] message (count LE | success bits of the ended episodes in order | spare)."""
    f = flags.reshape(-1)
    out = torch.empty(4 + cap + 1, dtype=U8, device=f.device) if out is None else out
    check(lib().uav_pack_success_bits(_h(f), _p(f, U8, name="flags"), f.numel(), int(cap), _p(out, U8, (4 + cap + 1,), "msg"),
                                      _stream()), "uav_pack_success_bits")
    return out


def episode_rows(rew, info, flags, carry, rows, count, env_offset=0):
    """uav_episode_rows: per-episode sums of the episodes that ended in this rollout, appended to rows [cap, 12] f64 in arbitrary
    order (count i32 [1], zeroed by the caller); carry f64 [N, 8] holds the episodes in progress."""
    N, T = rew.shape
    check(lib().uav_episode_rows(_h(rew), _p(rew, F32, (N, T), "rew"), _p(info, F32, (N, T, 10), "info"), _p(flags, U8, (N, T), "flags"),
                                 N, T, int(env_offset), _p(carry, torch.float64, (N, 8), "carry"),
                                 _p(rows, torch.float64, (rows.shape[0], 12), "rows"), int(rows.shape[0]), _p(count, I32, (1,), "count"),
                                 _stream()), "uav_episode_rows")


def curriculum_state(device, radius=50.0, bonus=0.6, bonus_is_f64=False):
    """A device-side curriculum state (uav_curriculum_*): opaque u8 block, initialised."""
    st = torch.zeros(int(lib().uav_curriculum_state_bytes()), dtype=U8, device=device)
    curriculum_init(st, radius, bonus, bonus_is_f64)
    return st


def curriculum_init(state, radius, bonus, bonus_is_f64=False):
    check(lib().uav_curriculum_init(_h(state), _p(state, U8, name="curriculum state"), float(radius), float(bonus), int(bool(bonus_is_f64)),
                                    _stream()), "uav_curriculum_init")


def curriculum_update(state, msgs, cap):
    """Feed the success messages of all ranks (u8 [world, 4 + cap + 1], uav_pack_success_bits) to the device-side curriculum."""
    world = int(msgs.shape[0])
    check(lib().uav_curriculum_update(_h(state), _p(state, U8, name="curriculum state"), _p(msgs, U8, (world, 4 + cap + 1), "msgs"), world,
                                      int(cap), _stream()), "uav_curriculum_update")


def curriculum_read(state_host):
    """Decode a HOST copy (numpy u8 / torch cpu u8) of a curriculum state -> dict."""
    import numpy as np
    b = np.asarray(state_host, dtype=np.uint8)
    d = b[:32].view(np.float64)
    q = b[32:48].view(np.int64)
    i = b[48:56].view(np.int32)
    return {"radius": float(d[0]), "bonus": float(d[1]), "bonus_is_f64": bool(d[2] != 0.0), "overflow": bool(d[3] != 0.0),
            "episodes": int(q[0]), "successes": int(q[1]), "hist_len": int(i[0]), "win_succ": int(i[1])}


# ----------------------------------------------------------------------------- U2 / K3
def ppo_loss(logits, value, act, logp_old, adv, ret, val_old, inv_n, clip, ent_beta,
             loss_sums=None, dlogits=None, dvalue=None, dhead_bias=None):
    n, A = logits.shape
    loss_sums = torch.empty(4, dtype=F64, device=logits.device) if loss_sums is None else loss_sums
    dlogits = torch.empty_like(logits) if dlogits is None else dlogits
    dvalue = torch.empty(n, dtype=F32, device=logits.device) if dvalue is None else dvalue
    check(lib().uav_ppo_loss(_h(logits), _p(logits, F32, (n, A), "logits"), _p(value.reshape(-1), F32, (n,), "value"),
                             _p(act, I32, (n,), "act"), _p(logp_old, F32, (n,), "logp_old"),
                             _p(adv, F32, (n,), "adv"), _p(ret, F32, (n,), "ret"), _p(val_old, F32, (n,), "val_old"),
                             n, A, float(inv_n), float(clip), float(ent_beta), _p(loss_sums, F64, (4,), "loss_sums"),
                             _p(dlogits, F32, (n, A), "dlogits"), _p(dvalue, F32, (n,), "dvalue"),
                             _p(dhead_bias, F32, (A + 1,), "dhead_bias"), _stream()),
          "uav_ppo_loss")
    return loss_sums, dlogits, dvalue


def policy_sample(logits, u=None, seed=0, counter=0, forced_act=None, want_probs=False, nan_count=None, index_offset=0,
                  iteration=0):
    """Row i draws from Philox(seed; counter, index_offset + i, iteration) -- uav_rollout's key when counter = the step
    inside the rollout, index_offset = the global index of this rank's first env."""
    n, A = logits.shape
    dev = logits.device
    act = torch.empty(n, dtype=I32, device=dev)
    logp = torch.empty(n, dtype=F32, device=dev)
    probs = torch.empty(n, A, dtype=F32, device=dev) if want_probs else None
    nan_count = torch.zeros(1, dtype=I32, device=dev) if nan_count is None else nan_count
    check(lib().uav_policy_sample(_h(logits), _p(logits, F32, (n, A), "logits"), n, A, _p(u, F32, (n,), "u"),
                                  int(seed), (int(iteration) << 32) | (int(counter) & 0xffffffff), int(index_offset),
                                  _p(forced_act, I32, (n,), "forced_act"),
                                  _p(act), _p(logp), _p(probs), _p(nan_count, I32, (1,), "nan_count"), _stream()),
          "uav_policy_sample")
    return act, logp, probs, nan_count


def policy_sample_at(heads_seq, t, act_out, act_buf, val_buf, logp_buf, nan_count, seed=0, iteration=0, index_offset=0,
                     forced_act=None):
    """policy_sample for time step t of a step-wise rollout: logits | value read from heads_seq[:, t] ([N, T, A+1]), the
    action also to act_out [N] (the env step's input), action / value / log-prob to column t of the [N, T] buffers."""
    N, T, A1 = heads_seq.shape
    check(lib().uav_policy_sample_at(_h(heads_seq), C.c_void_p(_p(heads_seq, F32, (N, T, A1), "heads_seq").value + 4 * int(t) * A1),
                                     T * A1, N, A1 - 1, int(seed), (int(iteration) << 32) | (int(t) & 0xffffffff),
                                     int(index_offset), _p(forced_act, I32, (N,), "forced_act"), _p(act_out, I32, (N,), "act_out"),
                                     T, int(t), _p(act_buf, I32, (N, T), "act_buf"), _p(val_buf, F32, (N, T), "val_buf"),
                                     _p(logp_buf, F32, (N, T), "logp_buf"), _p(nan_count, I32, (1,), "nan_count"), _stream()),
          "uav_policy_sample_at")
    return act_out


def store_transition(t, keep, rew, done, flags, keep_buf, rew_buf, done_buf, flags_buf):
    """PPOBuffer.store's remaining columns for step t: keep / rew / done / flags [N] -> column t of the [N, T] buffers;
    keep becomes 1 - done (the next step's restart mask)."""
    N, T = keep_buf.shape
    check(lib().uav_store_transition(_h(keep), N, T, int(t), _p(keep, F32, (N,), "keep"), _p(rew, F32, (N,), "rew"),
                                     _p(done, F32, (N,), "done"), _p(flags, U8, (N,), "flags"), _p(keep_buf, F32, (N, T), "keep_buf"),
                                     _p(rew_buf, F32, (N, T), "rew_buf"), _p(done_buf, F32, (N, T), "done_buf"),
                                     _p(flags_buf, U8, (N, T), "flags_buf"), _stream()), "uav_store_transition")


def rollout_tail(env_state, cfg, y_seq, t, w_head, b_head, heads_seq, act_out, cur_obs, obs_seq, keep, act_buf, val_buf, logp_buf,
                 keep_buf, rew_buf, done_buf, flags_buf, nan_count, seed=0, iteration=0, index_offset=0, forced_act=None, noise=None):
    """uav_rollout_tail: everything of rollout step t after the recurrent layers in one launch -- heads_seq[:, t] from
    y_seq[:, t] ([N, T, H] top-layer output), the action draw, the environment step (auto-reset), PPOBuffer.store's columns
    (act / val / logp / keep / rew / done / flags [N, T] at t; keep [N] <- 1 - done) and the next observation into cur_obs and
    obs_seq[:, t + 1].  Identical results to gemm_rows + policy_sample_at + env_step + store_transition + the obs copy."""
    N, T, H = y_seq.shape
    A1 = heads_seq.shape[-1]
    od = cur_obs.shape[-1]
    check(lib().uav_rollout_tail(_h(y_seq), _p(env_state, U8, name="env state"), N, C.byref(cfg),
                                 C.c_void_p(_p(y_seq, F32, (N, T, H), "y_seq").value + 4 * int(t) * H), T * H, H,
                                 _p(w_head, F32, (A1, H), "w_head"), _p(b_head, F32, (A1,), "b_head"), A1 - 1,
                                 C.c_void_p(_p(heads_seq, F32, (N, T, A1), "heads_seq").value + 4 * int(t) * A1), T * A1, T, int(t),
                                 int(seed), (int(iteration) << 32) | (int(t) & 0xffffffff), int(index_offset),
                                 _p(forced_act, I32, (N,), "forced_act"), _p(noise, F64, (N, 2), "noise"),
                                 _p(act_out, I32, (N,), "act_out"), _p(cur_obs, F32, (N, od), "cur_obs"),
                                 _p(obs_seq, F32, (N, T, od), "obs_seq"), _p(keep, F32, (N,), "keep"),
                                 _p(act_buf, I32, (N, T), "act_buf"), _p(val_buf, F32, (N, T), "val_buf"),
                                 _p(logp_buf, F32, (N, T), "logp_buf"), _p(keep_buf, F32, (N, T), "keep_buf"),
                                 _p(rew_buf, F32, (N, T), "rew_buf"), _p(done_buf, F32, (N, T), "done_buf"),
                                 _p(flags_buf, U8, (N, T), "flags_buf"), _p(nan_count, I32, (1,), "nan_count"), _stream()),
          "uav_rollout_tail")
    return act_out


def ppo_loss_heads(heads, act, logp_old, adv, ret, val_old, inv_n, clip, ent_beta, loss_sums, dheads, dhead_bias=None):
    """Packed form of ppo_loss: heads [n, A+1] (logits | value) in, dheads [n, A+1] out -- no split/concat copies."""
    n, A1 = heads.shape
    check(lib().uav_ppo_loss(_h(heads), _p(heads, F32, (n, A1), "heads"), None, _p(act, I32, (n,), "act"),
                             _p(logp_old, F32, (n,), "logp_old"), _p(adv, F32, (n,), "adv"), _p(ret, F32, (n,), "ret"),
                             _p(val_old, F32, (n,), "val_old"), n, A1 - 1, float(inv_n), float(clip), float(ent_beta),
                             _p(loss_sums, F64, (4,), "loss_sums"), _p(dheads, F32, (n, A1), "dheads"), None,
                             _p(dhead_bias, F32, (A1,), "dhead_bias"), _stream()), "uav_ppo_loss")
    return loss_sums, dheads


def ppo_loss_from_y(y, w_head, b_head, act, logp_old, adv, ret, val_old, inv_n, clip, ent_beta, loss_sums, dheads,
                    dhead_bias=None):
    """Heads + loss fused (csrc/loss.hip: ppo_loss_from_y_kernel): y [n, H] -> dheads [n, A+1]."""
    n, H = y.shape
    A1 = w_head.shape[0]
    _t = KERNEL_TIMER.bracket("ppo_loss")
    check(lib().uav_ppo_loss_from_y(_h(y), _p(y, F32, (n, H), "y"), _p(w_head, F32, (A1, H), "w_head"),
                                    _p(b_head, F32, (A1,), "b_head"), _p(act, I32, (n,), "act"),
                                    _p(logp_old, F32, (n,), "logp_old"), _p(adv, F32, (n,), "adv"),
                                    _p(ret, F32, (n,), "ret"), _p(val_old, F32, (n,), "val_old"), n, H, A1 - 1,
                                    float(inv_n), float(clip), float(ent_beta), _p(loss_sums, F64, (4,), "loss_sums"),
                                    _p(dheads, F32, (n, A1), "dheads"), _p(dhead_bias, F32, (A1,), "dhead_bias"),
                                    _stream()), "uav_ppo_loss_from_y")
    if _t is not None:
        _t.record()
    return loss_sums, dheads


BC_SUMS_N = 6              # UAV_BC_SUMS_N
# the six sums, include/uavppo.h uav_bc_loss
BC_SUMS_NAMES = ("nll", "value_loss", "entropy", "nan", "agree", "count")


def bc_loss_heads(heads, act, vtarget, inv_n, value_coef, ent_beta, bc_sums, dheads, dhead_bias=None):
    """Behaviour-cloning loss on packed heads (uav_bc_loss): heads [n, 6] (logits | value) and the expert's actions i32 [n] in,
    dheads [n, 6] and bc_sums f64 [BC_SUMS_N] out.  act outside 0 .. 4 masks a sample (zero row of dheads, in no sum);
    vtarget f32 [n] or None (no value regression)."""
    n, A1 = heads.shape
    check(lib().uav_bc_loss(_h(heads), _p(heads, F32, (n, A1), "heads"), _p(act, I32, (n,), "act"), _p(vtarget, F32, (n,), "vtarget"),
                            n, A1 - 1, float(inv_n), float(value_coef), float(ent_beta), _p(bc_sums, F64, (BC_SUMS_N,), "bc_sums"),
                            _p(dheads, F32, (n, A1), "dheads"), _p(dhead_bias, F32, (A1,), "dhead_bias"), _stream()), "uav_bc_loss")
    return bc_sums, dheads


PPO_DIAG_N = 8             # UAV_PPO_DIAG_N
# the eight sums, include/uavppo.h UAV_PPO_DIAG_*
PPO_DIAG_NAMES = ("kl_k1", "kl_k3", "clipped", "value_clipped", "verr2", "ret", "ret2", "count")


def set_ppo_diag(diag, device=None):
    """Attach a device f64 [PPO_DIAG_N] buffer to the device's handle (uav_set_ppo_diag): until set_ppo_diag(None) detaches it,
    every loss-bearing call on that device -- ppo_loss, ppo_loss_heads, ppo_loss_from_y, mlp_ppo_grad, mlp_ppo_grad_trend,
    mlp_ppo_grad_rows -- overwrites it with the call's eight diagnostic sums.  The handle keeps the POINTER: detach before the
    tensor is freed."""
    handle = Context.get(device).handle if diag is None else _h(diag)      # `device` says whose handle to detach from
    check(lib().uav_set_ppo_diag(handle, _p(diag, F64, (PPO_DIAG_N,), "diag")), "uav_set_ppo_diag")


# ----------------------------------------------------------------------------- U3
ARITH = {"fp16x3": 0, "bf16x6": 1, "f32_mfma": 2}


def set_lstm_arith(mode, device=None):
    """Operand arithmetic of the LSTM sequence kernels on this device's handle (include/uavppo.h, UAV_ARITH_*)."""
    check(lib().uav_set_lstm_arith(Context.get(device).handle, ARITH[mode]), "uav_set_lstm_arith")


class lstm_arith:
    """`with ops.lstm_arith("f32_mfma"):` -- run a block on another arithmetic, then restore the handle's mode."""

    def __init__(self, mode, device=None):
        self.mode, self.device = mode, device

    def __enter__(self):
        self.prev = get_lstm_arith(self.device)
        set_lstm_arith(self.mode, self.device)

    def __exit__(self, *exc):
        set_lstm_arith(self.prev, self.device)


DEBUG_FLAGS = {"step_f32": 1, "x_f32": 2, "dg_f32": 4, "gemm_tn_off": 0x10}


def set_debug_flags(*names, device=None):
    """A/B switches of the h = 256 step path on this device's handle (include/uavppo.h, UAV_DEBUG_*); no names = none."""
    check(lib().uav_set_debug_flags(Context.get(device).handle, sum(DEBUG_FLAGS[n] for n in names)), "uav_set_debug_flags")


# ---- K9: RCCL behind the ABI (csrc/comm.hip; include/uavppo.h "K9")
def rccl_version():
    """RCCL's version code (e.g. 22706) as the library the ABI binds reports it."""
    out = C.c_int(0)
    check(lib().uav_rccl_version(C.byref(out)), "uav_rccl_version")
    return int(out.value)


def comm_unique_id():
    """128 opaque bytes drawn by rank 0 (ncclGetUniqueId); hand them to every rank's comm_init over any host channel."""
    buf = C.create_string_buffer(128)
    check(lib().uav_comm_unique_id(buf), "uav_comm_unique_id")
    return bytes(buf.raw)


def comm_init(uid, rank, world, device=None):
    """Join the job's communicator with this device's handle (blocks until all `world` ranks have called it)."""
    if len(uid) != 128:
        raise RuntimeError("comm_init: the unique id is 128 bytes")
    check(lib().uav_comm_init(Context.get(device).handle, C.c_char_p(uid), int(rank), int(world)), "uav_comm_init")


def comm_world(device=None):
    return int(lib().uav_comm_world(Context.get(device).handle))


def comm_destroy(device=None):
    check(lib().uav_comm_destroy(Context.get(device).handle), "uav_comm_destroy")


def comm_allreduce(t):
    """In-place sum over the ranks on the current stream: f32 (the flat gradient) or f64 (advantage statistics, loss sums)."""
    if t.dtype == torch.float32:
        check(lib().uav_allreduce(_h(t), _p(t, F32, name="t"), t.numel(), _stream()), "uav_allreduce")
    elif t.dtype == torch.float64:
        check(lib().uav_allreduce_f64(_h(t), _p(t, torch.float64, name="t"), t.numel(), _stream()), "uav_allreduce_f64")
    else:
        raise RuntimeError(f"comm_allreduce: f32 or f64, got {t.dtype}")
    return t


def comm_allgather_bytes(msg):
    """[world, len(msg)] u8: every rank's message, in rank order."""
    w = comm_world(msg.device)
    if w < 1:
        raise RuntimeError("comm_allgather_bytes: no communicator on this device's handle")
    out = torch.empty(w, msg.numel(), dtype=torch.uint8, device=msg.device)
    check(lib().uav_allgather_bytes(_h(msg), _p(msg, torch.uint8, name="msg"), _p(out, torch.uint8, name="out"), msg.numel(), _stream()),
          "uav_allgather_bytes")
    return out


def get_lstm_arith(device=None):
    m = int(lib().uav_get_lstm_arith(Context.get(device).handle))
    return {v: k for k, v in ARITH.items()}[m]


def absmax(x, out=None):
    """max |x| (NaN -> inf) as a 1-element device tensor; no host sync."""
    out = torch.empty(1, dtype=F32, device=x.device) if out is None else out
    check(lib().uav_absmax(_h(x), _p(x, F32, name="x"), x.numel(), _p(out, F32, (1,), "out"), _stream()), "uav_absmax")
    return out


def clip_adam(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5,
              gnorm_out=None, pmax_out=None):
    n = param.numel()
    for t, nm in ((grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if t.numel() != n:
            raise RuntimeError(f"clip_adam: {nm} has {t.numel()} elements, param has {n}")
    check(lib().uav_clip_adam(_h(param), _p(param, F32, name="param"), _p(grad, F32, name="grad"),
                              _p(exp_avg, F32, name="exp_avg"), _p(exp_avg_sq, F32, name="exp_avg_sq"), n, int(step),
                              float(lr), float(beta1), float(beta2), float(eps), float(max_norm),
                              _p(gnorm_out, F32, (1,), "gnorm_out"), _p(pmax_out, F32, (1,), "pmax_out"), _stream()),
          "uav_clip_adam")


def clip_adam_dlr(param, grad, exp_avg, exp_avg_sq, step, lr_dev, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5,
                  gnorm_out=None, pmax_out=None):
    """clip_adam with the step size read from lr_dev (device f32 [1]) by the step kernel: clip_adam's bits for lr = lr_dev[0],
    with no host read of the rate (uav_clip_adam_dlr)."""
    n = param.numel()
    for t, nm in ((grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if t.numel() != n:
            raise RuntimeError(f"clip_adam_dlr: {nm} has {t.numel()} elements, param has {n}")
    if lr_dev is None:
        raise RuntimeError("clip_adam_dlr: lr_dev is a device f32 [1] tensor")
    check(lib().uav_clip_adam_dlr(_h(param), _p(param, F32, name="param"), _p(grad, F32, name="grad"),
                                  _p(exp_avg, F32, name="exp_avg"), _p(exp_avg_sq, F32, name="exp_avg_sq"), n, int(step),
                                  _p(lr_dev, F32, (1,), "lr_dev"), float(beta1), float(beta2), float(eps), float(max_norm),
                                  _p(gnorm_out, F32, (1,), "gnorm_out"), _p(pmax_out, F32, (1,), "pmax_out"), _stream()),
          "uav_clip_adam_dlr")


LR_STATE_N = 6             # UAV_LR_STATE_N
# the six slots, include/uavppo.h UAV_LR_STATE_*
LR_STATE_NAMES = ("lr", "last_kl", "raised", "lowered", "held", "skipped")


def lr_init(state, lr, lr_out=None):
    """L1: state f64 [LR_STATE_N] = {lr, 0, 0, 0, 0, 0}; returns lr_out f32 [1] = (float)lr.  No host sync."""
    lr_out = torch.empty(1, dtype=F32, device=state.device) if lr_out is None else lr_out
    check(lib().uav_lr_init(_h(state), _p(state, F64, (LR_STATE_N,), "state"), float(lr), _p(lr_out, F32, (1,), "lr_out"), _stream()),
          "uav_lr_init")
    return lr_out


def lr_adapt(state, diag8, desired_kl, factor, lr_min, lr_max, lr_out=None):
    """L2: one update's decision (lr_control.adapt_rule) on state f64 [LR_STATE_N], in place, from the all-reduced diagnostic
    sums diag8 f64 [PPO_DIAG_N] of the update's last epoch; returns lr_out f32 [1] = (float)lr.  No host sync."""
    lr_out = torch.empty(1, dtype=F32, device=state.device) if lr_out is None else lr_out
    check(lib().uav_lr_adapt(_h(state), _p(state, F64, (LR_STATE_N,), "state"), _p(diag8, F64, (PPO_DIAG_N,), "diag8"),
                             float(desired_kl), float(factor), float(lr_min), float(lr_max), _p(lr_out, F32, (1,), "lr_out"),
                             _stream()), "uav_lr_adapt")
    return lr_out


# ----------------------------------------------------------------------------- GEMM
def gemm_rows(a, b_t, bias, out):
    """out[n, :] = a[n, :] @ b_t.T + bias for ROW-STRIDED 2-D views a [N, K] and out [N, M] (unit stride along the last
    index, any row stride: one time step of an [N, T, K] array) and a contiguous b_t [M, K]: uav_gemm_f32 with lda / ldc."""
    N, K = a.shape
    M = b_t.shape[0]
    if a.stride(1) != 1 or out.stride(1) != 1 or tuple(out.shape) != (N, M) or b_t.shape[1] != K:
        raise RuntimeError("gemm_rows: a [N, K] and out [N, M] need unit stride along the last index; b_t is [M, K]")
    for t, nm in ((a, "a"), (out, "out")):
        if not t.is_cuda or t.dtype != F32:
            raise RuntimeError(f"gemm_rows: {nm}: expected a float32 GPU tensor")
    check(lib().uav_gemm_f32(_h(a), N, M, K, C.c_void_p(a.data_ptr()), a.stride(0), 1, _p(b_t, F32, name="b_t"), 1, K,
                             C.c_void_p(out.data_ptr()), out.stride(0), _p(bias, F32, (M,), "bias"), 0, _stream()),
          "uav_gemm_f32")
    return out


def gemm(a, b, trans_a=False, trans_b=False, bias=None, out=None, accumulate=False, split_fp16=False, a_absmax=None):
    """out[M,N] (+)= op(a) @ op(b) + bias with 2-D row-major tensors (op = optional transpose).  split_fp16: the same
    product as three fp16 piece products per f32 product (uav_gemm_f16x3: M % 128 == 0, N % 128 == 0, operands inside
    fp16's range; a_absmax = 1-element device tensor with max |a| block-scales a gradient-sized operand)."""
    if a.dim() != 2 or b.dim() != 2:
        raise RuntimeError("gemm: 2-D tensors expected")
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    K2, N = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if K != K2:
        raise RuntimeError(f"gemm: inner dimensions differ ({K} vs {K2})")
    sa_m, sa_k = (1, a.shape[1]) if trans_a else (a.shape[1], 1)
    sb_k, sb_n = (1, b.shape[1]) if trans_b else (b.shape[1], 1)
    if out is None:
        if accumulate:
            raise RuntimeError("gemm: accumulate needs out")
        out = torch.empty(M, N, dtype=F32, device=a.device)
    if split_fp16:
        check(lib().uav_gemm_f16x3(_h(a), M, N, K, _p(a, F32, name="a"), sa_m, sa_k, _p(b, F32, name="b"), sb_k, sb_n,
                                   _p(out, F32, (M, N), "out"), N, _p(bias, F32, (N,), "bias"), int(accumulate),
                                   _p(a_absmax, F32, (1,), "a_absmax"), _stream()), "uav_gemm_f16x3")
        return out
    check(lib().uav_gemm_f32(_h(a), M, N, K, _p(a, F32, name="a"), sa_m, sa_k, _p(b, F32, name="b"), sb_k, sb_n,
                             _p(out, F32, (M, N), "out"), N, _p(bias, F32, (N,), "bias"), int(accumulate), _stream()),
          "uav_gemm_f32")
    return out


# ----------------------------------------------------------------------------- M2
def mlp_param_count(in_dim=6, h1=256, h2=128, n_act=5):
    return int(lib().uav_mlp_param_count(in_dim, h1, h2, n_act))


def mlp_fwd(params, x, in_dim=6, h1=256, h2=128, n_act=5, stash=None):
    B = x.shape[0]
    if params.numel() != mlp_param_count(in_dim, h1, h2, n_act):
        raise RuntimeError("mlp_fwd: flat parameter buffer has the wrong size")
    heads = torch.empty(B, n_act + 1, dtype=F32, device=x.device)
    per = int(lib().uav_mlp_stash_floats(h1, h2))
    if stash is None:
        stash = torch.empty(B * per, dtype=F32, device=x.device)
    elif stash.numel() < B * per:
        raise RuntimeError("mlp_fwd: stash too small")
    check(lib().uav_mlp_fwd(_h(x), _p(params, F32, name="params"), _p(x, F32, (B, in_dim), "x"), B, in_dim, h1, h2,
                            n_act, _p(heads), _p(stash, F32, name="stash"), _stream()), "uav_mlp_fwd")
    return heads, stash


def mlp_bwd(params, x, stash, dheads, in_dim=6, h1=256, h2=128, n_act=5, grad=None):
    B = x.shape[0]
    grad = torch.empty_like(params) if grad is None else grad
    check(lib().uav_mlp_bwd(_h(x), _p(params, F32, name="params"), _p(x, F32, (B, in_dim), "x"),
                            _p(stash, F32, name="stash"), _p(dheads, F32, (B, n_act + 1), "dheads"), B, in_dim, h1,
                            h2, n_act, _p(grad, F32, params.shape, "grad"), _stream()), "uav_mlp_bwd")
    return grad


def mlp_ppo_grad(params, obs, act, logp_old, adv, ret, val_old, inv_n, clip, ent_beta, loss_sums, grad, in_dim=6, h1=256,
                 h2=128, n_act=5):
    """Fused forward + clipped-PPO loss + backward of the reference's MLP policy (csrc/mlp_update.hip): obs [n, 6] and the
    per-sample scalars in, flat gradient (layout of `params`) and loss_sums f64[4] out; nothing else touches HBM."""
    n = obs.shape[0]
    _t = KERNEL_TIMER.bracket("mlp_ppo_grad")
    check(lib().uav_mlp_ppo_grad(_h(obs), _p(params, F32, (mlp_param_count(in_dim, h1, h2, n_act),), "params"),
                                 _p(obs, F32, (n, in_dim), "obs"), _p(act, I32, (n,), "act"),
                                 _p(logp_old, F32, (n,), "logp_old"), _p(adv, F32, (n,), "adv"), _p(ret, F32, (n,), "ret"),
                                 _p(val_old, F32, (n,), "val_old"), n, in_dim, h1, h2, n_act, float(inv_n), float(clip),
                                 float(ent_beta), _p(loss_sums, F64, (4,), "loss_sums"), _p(grad, F32, params.shape, "grad"),
                                 _stream()), "uav_mlp_ppo_grad")
    if _t is not None:
        _t.record()
    return grad


class GatherPlan:
    """The checked arguments of gather_rows_multi for one fixed set of (src, dst) arrays: built once, launched many times
    (the trainer's packed minibatch buffers never move).  Keeps the tensors alive."""

    def __init__(self, pairs):
        pairs = [tuple(p) for p in pairs]
        if not 1 <= len(pairs) <= _lib.GATHER_MAX_SPECS:
            raise RuntimeError(f"gather_rows_multi: {len(pairs)} arrays (1 .. {_lib.GATHER_MAX_SPECS})")
        self.specs = (_lib.GatherSpec * len(pairs))()
        self.tensors = pairs
        self.n_rows = self.max_sel = None
        for k, pair in enumerate(pairs):
            src, dst = pair[:2]
            rd = int(pair[2]) if len(pair) > 2 else 0          # the dimension the rows are selected on: 0, or 1 behind a plane dimension
            name = f"pairs[{k}]"
            _p(src, name=name + " src")
            _p(dst, src.dtype, name=name + " dst")
            if rd not in (0, 1) or src.dim() <= rd or dst.dim() != src.dim():
                raise RuntimeError(f"{name}: row dimension {rd} of shapes {tuple(src.shape)} -> {tuple(dst.shape)}")
            if src.shape[:rd] != dst.shape[:rd] or src.shape[rd + 1:] != dst.shape[rd + 1:]:
                raise RuntimeError(f"{name}: shapes {tuple(src.shape)} -> {tuple(dst.shape)} differ outside the row dimension")
            row_bytes = src[(0,) * (rd + 1)].numel() * src.element_size()
            if row_bytes == 0 or row_bytes % 4:
                raise RuntimeError(f"{name}: rows of {row_bytes} bytes (a positive multiple of 4)")
            if self.n_rows not in (None, src.shape[rd]):
                raise RuntimeError(f"{name}: {src.shape[rd]} source rows, the arrays before it have {self.n_rows}")
            self.n_rows = int(src.shape[rd])
            self.max_sel = int(dst.shape[rd]) if self.max_sel is None else min(self.max_sel, int(dst.shape[rd]))
            planes = int(src.shape[0]) if rd else 1
            self.specs[k] = _lib.GatherSpec(src.data_ptr(), dst.data_ptr(), row_bytes, planes, 0, self.n_rows * row_bytes,
                                            int(dst.shape[rd]) * row_bytes)
        self.handle = _h(pairs[0][0])


def gather_rows_multi(idx, pairs):
    """uav_gather_rows_multi: dst[j] = src[idx[j]] for every (src, dst) of `pairs` in ONE launch -- the bytes of
    torch.index_select(src, 0, idx) in dst[:len(idx)].  idx i32 [n_sel]; a pair is (src [n_rows, ...], dst [>= n_sel, ...]) or,
    for arrays with a leading plane dimension such as h0 [L, N, H], (src, dst, 1): dst[p, j] = src[p, idx[j]].  Rows of dst
    past n_sel are left alone.  4-byte-multiple rows, same dtype per pair, at most 12 pairs.  `pairs` may be a GatherPlan built
    from them before.  An index outside [0, n_rows) is clamped by the kernel."""
    plan = pairs if isinstance(pairs, GatherPlan) else GatherPlan(pairs)
    if idx.dim() != 1 or not 1 <= idx.numel() <= plan.max_sel:
        raise RuntimeError(f"gather_rows_multi: idx of shape {tuple(idx.shape)} for destinations of {plan.max_sel} rows")
    _t = KERNEL_TIMER.bracket("gather_rows")
    check(lib().uav_gather_rows_multi(plan.handle, _p(idx, I32, name="idx"), idx.numel(), plan.n_rows, plan.specs, len(plan.specs),
                                      _stream()), "uav_gather_rows_multi")
    if _t is not None:
        _t.record()
    return plan


def mlp_ppo_grad_trend(params, obs, act, logp_old, adv, ret, val_old, inv_n, clip, ent_beta, loss_sums, grad, trend_k):
    """mlp_ppo_grad for an MLP that takes the trend channels as inputs (uav_mlp_ppo_grad_trend): obs [n, 6 + trend_k],
    params / grad of mlp_param_count(6 + trend_k) floats, trend_k 0, 1 or 2 (0 is mlp_ppo_grad's kernel and bits)."""
    n, D = obs.shape[0], 6 + int(trend_k)
    _mlp_trend_params("mlp_ppo_grad_trend", params, trend_k)
    _t = KERNEL_TIMER.bracket("mlp_ppo_grad")
    check(lib().uav_mlp_ppo_grad_trend(_h(obs), _p(params, F32, name="params"), _p(obs, F32, (n, D), "obs"),
                                       _p(act, I32, (n,), "act"), _p(logp_old, F32, (n,), "logp_old"), _p(adv, F32, (n,), "adv"),
                                       _p(ret, F32, (n,), "ret"), _p(val_old, F32, (n,), "val_old"), n, int(trend_k), float(inv_n),
                                       float(clip), float(ent_beta), _p(loss_sums, F64, (4,), "loss_sums"),
                                       _p(grad, F32, params.shape, "grad"), _stream()), "uav_mlp_ppo_grad_trend")
    if _t is not None:
        _t.record()
    return grad


def mlp_ppo_grad_rows(params, obs, act, logp_old, adv, ret, val_old, rows, inv_n, clip, ent_beta, loss_sums, grad, trend_k=0):
    """mlp_ppo_grad_trend over a minibatch of rows (uav_mlp_ppo_grad_rows): the six arrays hold n_total samples, rows i32
    [n_rows] indexes them, sample s of the launch is buffer row rows[s].  Bit-identical to the contiguous entries on gathered
    copies of the same rows in the same order; an index outside [0, n_total) is clamped by the kernel."""
    n_total, D = obs.shape[0], 6 + int(trend_k)
    _mlp_trend_params("mlp_ppo_grad_rows", params, trend_k)
    if rows.dim() != 1 or rows.numel() == 0:
        raise RuntimeError(f"mlp_ppo_grad_rows: rows must be a non-empty 1-d index tensor, got shape {tuple(rows.shape)}")
    if n_total >= 2 ** 31:
        raise RuntimeError(f"mlp_ppo_grad_rows: {n_total} buffer rows do not fit the i32 indices")
    _t = KERNEL_TIMER.bracket("mlp_ppo_grad")
    check(lib().uav_mlp_ppo_grad_rows(_h(obs), _p(params, F32, name="params"), _p(obs, F32, (n_total, D), "obs"),
                                      _p(act, I32, (n_total,), "act"), _p(logp_old, F32, (n_total,), "logp_old"),
                                      _p(adv, F32, (n_total,), "adv"), _p(ret, F32, (n_total,), "ret"),
                                      _p(val_old, F32, (n_total,), "val_old"), n_total, _p(rows, I32, name="rows"), rows.numel(),
                                      int(trend_k), float(inv_n), float(clip), float(ent_beta), _p(loss_sums, F64, (4,), "loss_sums"),
                                      _p(grad, F32, params.shape, "grad"), _stream()), "uav_mlp_ppo_grad_rows")
    if _t is not None:
        _t.record()
    return grad


def mlp_bc_grad(params, obs, act, vtarget, inv_n, value_coef, ent_beta, bc_sums, grad, trend_k=0, rows=None):
    """Fused forward + behaviour-cloning loss + backward of the 6+k-256-128 MLP (uav_mlp_bc_grad): obs [n_total, 6 + trend_k], act
    i32 [n_total], vtarget f32 [n_total] or None; rows None: all samples in order, rows i32 [n_rows]: sample s of the launch is
    buffer row rows[s] (clamped into the buffer by the kernel), bit-identical to the contiguous form on gathered copies.  Flat
    gradient and bc_sums f64 [BC_SUMS_N] out."""
    n_total, D = obs.shape[0], 6 + int(trend_k)
    _mlp_trend_params("mlp_bc_grad", params, trend_k)
    if rows is not None and (rows.dim() != 1 or rows.numel() == 0):
        raise RuntimeError(f"mlp_bc_grad: rows must be a non-empty 1-d index tensor, got shape {tuple(rows.shape)}")
    if n_total >= 2 ** 31:
        raise RuntimeError(f"mlp_bc_grad: {n_total} buffer rows do not fit the i32 indices")
    _t = KERNEL_TIMER.bracket("mlp_bc_grad")
    check(lib().uav_mlp_bc_grad(_h(obs), _p(params, F32, name="params"), _p(obs, F32, (n_total, D), "obs"),
                                _p(act, I32, (n_total,), "act"), _p(vtarget, F32, (n_total,), "vtarget"), n_total,
                                _p(rows, I32, name="rows"), 0 if rows is None else rows.numel(), int(trend_k), float(inv_n),
                                float(value_coef), float(ent_beta), _p(bc_sums, F64, (BC_SUMS_N,), "bc_sums"),
                                _p(grad, F32, params.shape, "grad"), _stream()), "uav_mlp_bc_grad")
    if _t is not None:
        _t.record()
    return grad


def _mlp_trend_params(who, params, trend_k):
    """The C ABI cannot see how long `params` is: a 6-input vector read as an 8-input network runs 512 floats past its end."""
    if not 0 <= int(trend_k) <= 2:
        raise RuntimeError(f"{who}: trend_k={trend_k} (the fused MLP kernels take 6 + trend_k inputs, trend_k 0, 1 or 2)")
    want = mlp_param_count(6 + int(trend_k))
    if params.numel() != want:
        raise RuntimeError(f"{who}: params has {params.numel()} floats, an MLP with {6 + int(trend_k)} inputs "
                           f"(trend_k = {int(trend_k)}) has {want}")


# ----------------------------------------------------------------------------- E1-E5
ENV_VARIANTS = {"v2.0": 0, "v2.1": 1, "v1.1": 2}
ENV_MAX_STEPS = {"v2.0": 1000, "v2.1": 1000, "v1.1": 5000}


def env_state_bytes(n_env):
    return int(lib().uav_env_state_bytes(int(n_env)))


def make_env_cfg(variant, radius, bonus, seed=0, bank=None, bank_src=None, env_offset=0, n_env_total=0, trend_k=0, curriculum=None):
    """uav_env_cfg (host struct).  bonus: python float -> the reference's f32 expression,
    numpy.float64 -> its f64 expression (see csrc/env_core.h, environment.py:133)."""
    import numpy as np
    cfg = EnvCfg()
    cfg.variant = ENV_VARIANTS[variant]
    cfg.field_mode = 1 if bank is not None else 0
    cfg.n_fields = 0 if bank is None else int(bank.shape[0])
    cfg.bonus_is_f64 = int(isinstance(bonus, np.float64))
    cfg.env_offset = int(env_offset)
    cfg.n_env_total = int(n_env_total)
    cfg.trend_k = int(trend_k)
    cfg.radius = float(radius)
    cfg.bonus = float(bonus)
    cfg.seed = int(seed)
    cfg.curriculum = None if curriculum is None else _p(curriculum, U8, name="curriculum state").value
    if bank is not None:
        F_ = bank.shape[0]
        cfg.bank = _p(bank, F64, (F_, 500, 500, 2), "bank").value
        cfg.bank_src = _p(bank_src, F64, (F_, 2), "bank_src").value
    return cfg


def env_reset(state, n_env, cfg, obs_out):
    check(lib().uav_env_reset(_h(state), _p(state, U8, name="env state"), n_env, C.byref(cfg),
                              _p(obs_out, F32, (n_env, 6 + cfg.trend_k), "obs_out"), _stream()), "uav_env_reset")


def env_step(state, n_env, cfg, act, obs_out, rew, done, flags, noise=None, info=None, term_obs=None, rew64=None):
    check(lib().uav_env_step(_h(state), _p(state, U8, name="env state"), n_env, C.byref(cfg),
                             _p(act, I32, (n_env,), "act"), _p(noise, F64, (n_env, 2), "noise"),
                             _p(obs_out, F32, (n_env, 6 + cfg.trend_k), "obs_out"), _p(rew, F32, (n_env,), "rew"),
                             _p(done, F32, (n_env,), "done"), _p(flags, U8, (n_env,), "flags"),
                             _p(info, F32, (n_env, 5), "info"), _p(term_obs, F32, (n_env, 6 + cfg.trend_k), "term_obs"),
                             _p(rew64, F64, (n_env,), "rew64"), _stream()), "uav_env_step")


def env_peek(state, n_env, pos=None, source=None, steps=None, episode=None):
    check(lib().uav_env_peek(_h(state), _p(state, U8, name="env state"), n_env, _p(pos, F32, (n_env, 2), "pos"),
                             _p(source, F64, (n_env, 2), "source"), _p(steps, I32, (n_env,), "steps"),
                             _p(episode, I32, (n_env,), "episode"), _stream()), "uav_env_peek")


# ----------------------------------------------------------------------------- L1
def lstm_fwd(x, keep, h0, c0, w_ih, w_hh, b_ih, b_hh, stash=None, want_stash=True, y=None, w_head=None, b_head=None,
             heads=None):
    """One nn.LSTM layer over x[N,T,I] (env-major).  Returns y[N,T,H], hn, cn, stash[N,T,6H].
    With w_head [A1,H], b_head [A1] and a heads [N,T,A1] buffer the kernel also writes heads = y W_head^T + b_head."""
    N, T, I = x.shape
    H = w_hh.shape[1]
    dev = x.device
    y = torch.empty(N, T, H, dtype=F32, device=dev) if y is None else y
    hn = torch.empty(N, H, dtype=F32, device=dev)
    cn = torch.empty(N, H, dtype=F32, device=dev)
    if stash is None and (want_stash or I > 8 or H not in (64, 128)):     # the non-fused / generic paths work through the stash
        stash = torch.empty(N, T, 6 * H, dtype=F32, device=dev)
    _t = KERNEL_TIMER.bracket("lstm_fwd")
    check(lib().uav_lstm_fwd(_h(x), _p(x, F32, (N, T, I), "x"), _p(keep, F32, (N, T), "keep"),
                             _p(h0, F32, (N, H), "h0"), _p(c0, F32, (N, H), "c0"), _p(w_ih, F32, (4 * H, I), "w_ih"),
                             _p(w_hh, F32, (4 * H, H), "w_hh"), _p(b_ih, F32, (4 * H,), "b_ih"),
                             _p(b_hh, F32, (4 * H,), "b_hh"), N, T, I, H, _p(y, F32, (N, T, H), "y"), _p(hn), _p(cn),
                             _p(stash, F32, (N, T, 6 * H), "stash"),
                             _p(w_head, F32, None if w_head is None else (w_head.shape[0], H), "w_head"),
                             _p(b_head, F32, None if w_head is None else (w_head.shape[0],), "b_head"),
                             0 if w_head is None else int(w_head.shape[0]),
                             _p(heads, F32, None if w_head is None else (N, T, w_head.shape[0]), "heads"), _stream()),
          "uav_lstm_fwd")
    if _t is not None:
        _t.record()
    return y, hn, cn, stash


def lstm_chunk_states(y, stash, keep, h0, c0, chunk, h_out=None, c_out=None):
    """uav_lstm_chunk_states: the state entering every chunk of `chunk` steps of one layer's forward pass, already masked.
    y [N, T, H], stash [N, T, 6H], keep [N, T] or None, h0, c0 [N, H] -> h_out, c_out [N * (T // chunk), H] (row n * C + k:
    chunk k of env n).  The outputs may be views into larger arrays (contiguous, any 4-byte alignment)."""
    N, T, H = y.shape
    chunk = int(chunk)
    rows = N * (T // chunk) if chunk >= 1 else 0
    h_out = torch.empty(rows, H, dtype=F32, device=y.device) if h_out is None else h_out
    c_out = torch.empty(rows, H, dtype=F32, device=y.device) if c_out is None else c_out
    check(lib().uav_lstm_chunk_states(_h(y), _p(y, F32, (N, T, H), "y"), _p(stash, F32, (N, T, 6 * H), "stash"),
                                      _p(keep, F32, (N, T), "keep"), _p(h0, F32, (N, H), "h0"), _p(c0, F32, (N, H), "c0"),
                                      N, T, H, chunk, _p(h_out, F32, (rows, H), "h_out"), _p(c_out, F32, (rows, H), "c_out"),
                                      _stream()), "uav_lstm_chunk_states")
    return h_out, c_out


class LstmStepper:
    """uav_lstm_fwd one time step per call for one layer (H = 256, fp16-split arithmetic): weights split once by begin(),
    recurrent state kept on the device in `state`; step(t) reads x[:, t] and fills y[:, t] / stash[:, t] of the [N, T]
    arrays the BPTT reads; its `keep` argument restarts the state of the envs whose episode ended in the previous step."""

    def __init__(self, N, I, H, device):
        nbytes = lib().uav_lstm_stepper_bytes(int(N), int(I), int(H))
        if nbytes == 0:
            raise RuntimeError(f"uav_lstm_stepper: N={N} I={I} H={H} not supported (H = 256, I <= 256)")
        self.N, self.I, self.H = int(N), int(I), int(H)
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.hn = torch.empty(N, H, dtype=F32, device=device)
        self.cn = torch.empty(N, H, dtype=F32, device=device)

    def begin(self, w_ih, w_hh, b_ih, b_hh, h0, c0):
        N, I, H = self.N, self.I, self.H
        check(lib().uav_lstm_stepper_begin(_h(self.state), _p(self.state), _p(w_ih, F32, (4 * H, I), "w_ih"),
                                           _p(w_hh, F32, (4 * H, H), "w_hh"), _p(b_ih, F32, (4 * H,), "b_ih"),
                                           _p(b_hh, F32, (4 * H,), "b_hh"), _p(h0, F32, (N, H), "h0"), _p(c0, F32, (N, H), "c0"),
                                           N, I, H, _stream()), "uav_lstm_stepper_begin")

    def step(self, x, t, y, stash, below=None, keep=None):
        """keep: [N] restart mask of this step (0 where the env's episode ended in the previous step) or None.
        below: the LstmStepper of the layer below, already stepped to t (x is then its y array: the kernel reads h_t from
        that stepper's piece planes instead of gathering and splitting f32 rows)."""
        N, I, H = self.N, self.I, self.H
        T = x.shape[1]
        check(lib().uav_lstm_stepper_step(_h(self.state), _p(self.state), _p(x, F32, (N, T, I), "x"),
                                          None if below is None else _p(below.state), _p(keep, F32, (N,), "keep"), N, T, int(t),
                                          I, H, _p(y, F32, (N, T, H), "y"), _p(stash, F32, (N, T, 6 * H), "stash"), _p(self.hn),
                                          _p(self.cn), _stream()), "uav_lstm_stepper_step")


def _stepper_call(sp, x, t, y, stash, below, keep):
    N, I, H = sp.N, sp.I, sp.H
    T = x.shape[1]
    c = _lib.StepperCall()
    c.state = _p(sp.state).value
    c.x = _p(x, F32, (N, T, I), "x").value
    c.below = None if below is None else _p(below.state).value
    c.keep_t = None if keep is None else _p(keep, F32, (N,), "keep").value
    c.t, c.I = int(t), I
    c.y = _p(y, F32, (N, T, H), "y").value
    c.stash = _p(stash, F32, (N, T, 6 * H), "stash").value
    c.hn, c.cn = _p(sp.hn).value, _p(sp.cn).value
    return c


def lstm_stepper_step_pair(a, b):
    """uav_lstm_stepper_step_pair: two INDEPENDENT stepper steps as one launch.  a, b: (stepper, x, t, y, stash, below, keep) as for
    LstmStepper.step -- e.g. layer 1's step t + 1 and layer 2's step t (below = layer 1's stepper)."""
    ca, cb = _stepper_call(*a), _stepper_call(*b)
    sp, x = a[0], a[1]
    check(lib().uav_lstm_stepper_step_pair(_h(sp.state), C.byref(ca), C.byref(cb), sp.N, x.shape[1], sp.H, _stream()),
          "uav_lstm_stepper_step_pair")


def lstm_dgates_bytes(N, T, H, device):
    """uav_lstm_dgates_bytes: size of the gate-gradient buffer uav_lstm_bwd / _bwd_stack hand to uav_lstm_wgrad under the device
    handle's CURRENT arithmetic mode and debug flags."""
    n = int(lib().uav_lstm_dgates_bytes(Context.get(torch.device(device)).handle, int(N), int(T), int(H)))
    if n <= 0:
        raise RuntimeError(f"uav_lstm_dgates_bytes({N}, {T}, {H}) = {n}")
    return n


def lstm_dgates(N, T, H, device):
    """A gate-gradient buffer for lstm_bwd / lstm_bwd_stack / lstm_wgrad: f32 rows [N, T, 4H] -- except at h = 256 on the fp16-split
    arithmetic, where the library keeps the BPTT's fp16 piece chunks + one scale per (env, step) instead of f32 rows and the
    buffer is an opaque flat f32 tensor (lstm_dgates_f32 converts)."""
    nbytes = lstm_dgates_bytes(N, T, H, device)
    if nbytes == N * T * 4 * H * 4:
        return torch.empty(N, T, 4 * H, dtype=F32, device=device)
    return torch.empty((nbytes + 3) // 4, dtype=F32, device=device)


def _pdg(dgates, N, T, H):
    need = lstm_dgates_bytes(N, T, H, dgates.device)
    if dgates.numel() * 4 < need:
        raise RuntimeError(f"dgates: {dgates.numel() * 4} bytes, uav_lstm_dgates_bytes({N}, {T}, {H}) = {need} (allocate with ops.lstm_dgates)")
    return _p(dgates, F32, None, "dgates")


def lstm_dgates_f32(dgates, N, T, H):
    """uav_lstm_dgates_f32: the gate gradients as f32 rows [N, T, 4H], whatever form the buffer holds them in."""
    out = torch.empty(N, T, 4 * H, dtype=F32, device=dgates.device)
    check(lib().uav_lstm_dgates_f32(_h(dgates), _pdg(dgates, N, T, H), N, T, H, _p(out), _stream()), "uav_lstm_dgates_f32")
    return out


DG_ROWS, DG_PIECES, DG_TILE_ARMED, DG_TILE = 0, 1, 2, 3      # uav_lstm_dgates_form (include/uavppo.h: UAV_DG_*)


def lstm_dgates_tile_bytes(N, T, I, H, device):
    """uav_lstm_dgates_tile_bytes: size of an h = 64 / 128 gate-gradient buffer in TILE form (the 16 rows a BPTT workgroup writes in
    a step adjacent; include/uavppo.h), or 0 when the library refuses the form for this shape and the caller keeps f32 rows."""
    return int(lib().uav_lstm_dgates_tile_bytes(Context.get(torch.device(device)).handle, int(N), int(T), int(I), int(H)))


def lstm_dgates_tile(N, T, I, H, device):
    """A gate-gradient buffer large enough for tile form (an opaque flat f32 tensor; pass it to lstm_bwd with dgates_tile), or None
    when the form is refused for this shape."""
    nbytes = lstm_dgates_tile_bytes(N, T, I, H, device)
    return torch.empty(nbytes // 4, dtype=F32, device=device) if nbytes else None


def lstm_dgates_form(dgates):
    """uav_lstm_dgates_form: DG_ROWS / DG_PIECES / DG_TILE_ARMED / DG_TILE as the device handle has recorded it for this buffer."""
    return int(lib().uav_lstm_dgates_form(_h(dgates), _p(dgates, F32, None, "dgates")))


def lstm_dgates_forget(dgates):
    """uav_lstm_dgates_forget: drop the handle's tile-form record of this buffer (before it is freed or filled by hand)."""
    check(lib().uav_lstm_dgates_forget(_h(dgates), _p(dgates, F32, None, "dgates")), "uav_lstm_dgates_forget")


def _arm_tile(dgates, N, T, I, H):
    need = lstm_dgates_tile_bytes(N, T, I, H, dgates.device)
    if not need:
        raise RuntimeError(lib().uav_last_error().decode())
    if dgates.numel() * 4 < need:
        raise RuntimeError(f"dgates: {dgates.numel() * 4} bytes, uav_lstm_dgates_tile_bytes({N}, {T}, {I}, {H}) = {need} (allocate with ops.lstm_dgates_tile)")
    check(lib().uav_lstm_dgates_tile(_h(dgates), _p(dgates, F32, None, "dgates"), N, T, I, H), "uav_lstm_dgates_tile")


@contextlib.contextmanager
def _tile_request(dgates, mode, N, T, I, H):
    """lstm_bwd's dgates_tile in one place: arm the buffer; if uav_lstm_bwd refuses (`written` still unset), forget it -- a refused
    call leaves the buffer as it was, f32 rows to whoever uses it next; and once the weight gradients are formed, forget a
    "transient" request (a work buffer nobody reads afterwards).  mode False: nothing at all."""
    request = types.SimpleNamespace(written=False)
    if mode:
        _arm_tile(dgates, N, T, I, H)
    try:
        yield request
    except Exception:
        if mode and not request.written:
            lstm_dgates_forget(dgates)
        raise
    if mode == "transient":
        lstm_dgates_forget(dgates)


def lstm_wgrad(x, keep, h0, y, stash, dgates, w_ih, dheads=None):
    """The weight-gradient pass alone, from given gate gradients: dW_ih, dW_hh, db (and dW_head = dheads^T y)."""
    N, T, I = x.shape
    H = y.shape[-1]
    dev = x.device
    nh = 0 if dheads is None else dheads.shape[-1]
    dw_ih = torch.empty(4 * H, I, dtype=F32, device=dev)
    dw_hh = torch.empty(4 * H, H, dtype=F32, device=dev)
    db = torch.empty(4 * H, dtype=F32, device=dev)
    dw_head = torch.empty(nh, H, dtype=F32, device=dev) if nh else None
    check(lib().uav_lstm_wgrad(_h(x), _p(x, F32, (N, T, I), "x"), _p(keep, F32, (N, T), "keep"), _p(h0, F32, (N, H), "h0"),
                               _p(y, F32, (N, T, H), "y"), _p(stash, F32, (N, T, 6 * H), "stash"),
                               _pdg(dgates, N, T, H), _p(w_ih, F32, (4 * H, I), "w_ih"),
                               _p(dheads, F32, (N, T, nh), "dheads"), nh, N, T, I, H,
                               _p(dw_ih, F32, (4 * H, I), "dw_ih"), _p(dw_hh, F32, (4 * H, H), "dw_hh"),
                               _p(db, F32, (4 * H,), "db"), None, _p(dw_head, F32, (nh, H), "dw_head"), _p(None), _stream()),
          "uav_lstm_wgrad")
    return {"dw_ih": dw_ih, "dw_hh": dw_hh, "db": db, "dw_head": dw_head}


def lstm_bwd_caps(device, I, H):
    """uav_lstm_bwd_caps bit mask for a layer of input width I, hidden size H on `device`: 1 = forms dx itself, 2 = takes
    dheads + w_head instead of dy."""
    return int(lib().uav_lstm_bwd_caps(Context.get(torch.device(device)).handle, int(I), int(H)))


def lstm_bwd_stack(layers, keep, dy=None, dheads=None, w_head=None):
    """uav_lstm_bwd_stack: the BPTTs of a stack of h = 256 layers as one pipelined call.  layers: top first, dicts with
    stash [N,T,6H], w_hh, w_ih (None for the last), dgates (ops.lstm_dgates; distinct per layer), dx [N,T,H] (None for the last)."""
    N, T, H6 = layers[0]["stash"].shape
    H = H6 // 6
    arr = (_lib.LstmBwdLayer * len(layers))()
    for a, d in zip(arr, layers):
        a.keep = None if keep is None else _p(keep, F32, (N, T), "keep").value
        a.stash = _p(d["stash"], F32, (N, T, 6 * H), "stash").value
        a.w_hh = _p(d["w_hh"], F32, (4 * H, H), "w_hh").value
        a.w_ih = None if d.get("w_ih") is None else _p(d["w_ih"], F32, (4 * H, H), "w_ih").value
        a.dgates = _pdg(d["dgates"], N, T, H).value
        a.dx = None if d.get("dx") is None else _p(d["dx"], F32, (N, T, H), "dx").value
        a.dhn = a.dcn = a.dh0 = a.dc0 = None
    nh = 0 if dheads is None else dheads.shape[-1]
    _t = KERNEL_TIMER.bracket("lstm_bwd")
    check(lib().uav_lstm_bwd_stack(_h(layers[0]["stash"]), len(layers), C.byref(arr), _p(dy, F32, (N, T, H), "dy"),
                                   _p(dheads, F32, (N, T, nh), "dheads"), _p(w_head, F32, (nh, H), "w_head"), nh, N, T, H, _stream()),
          "uav_lstm_bwd_stack")
    if _t is not None:
        _t.record()


def lstm_bwd(x, keep, stash, w_ih, w_hh, y, h0, dy=None, dheads=None, w_head=None, dhn=None, dcn=None, need_dx=False,
             dgates=None, dw_ih=None, dw_hh=None, db=None, dw_head=None, want_dstate=True, wgrad_dheads=None, bwd_done=False,
             db_hh=None, dgates_tile=False):
    """BPTT sequence kernel + fused weight-gradient pass of one layer.  y, h0: the layer's forward
    output and initial hidden state (h_prev of the weight gradient is y shifted by one step).
    db_hh: a second [4H] tensor that receives the bias gradient too (nn.LSTM's bias_hh; saves the caller a copy launch).
    bwd_done: dgates (and the dx a layer above needs) were already produced by lstm_bwd_stack: only the weight gradients.
    dgates_tile: the caller's `dgates` (ops.lstm_dgates_tile) is written and read in tile form, for this call alone -- same results
    to the bit; raises where the library refuses the form.  True leaves the buffer recorded as tile form (lstm_dgates_f32 returns its
    rows), "transient" drops the record once the weight gradients are formed (a work buffer nobody reads afterwards)."""
    N, T, I = x.shape
    H = w_hh.shape[1]
    dev = x.device
    dgates = lstm_dgates(N, T, H, dev) if dgates is None else dgates
    dx = torch.empty(N, T, I, dtype=F32, device=dev) if (need_dx and not bwd_done) else None
    dw_ih = torch.empty(4 * H, I, dtype=F32, device=dev) if dw_ih is None else dw_ih
    dw_hh = torch.empty(4 * H, H, dtype=F32, device=dev) if dw_hh is None else dw_hh
    db = torch.empty(4 * H, dtype=F32, device=dev) if db is None else db
    dh0 = torch.empty(N, H, dtype=F32, device=dev) if want_dstate else None
    dc0 = torch.empty(N, H, dtype=F32, device=dev) if want_dstate else None
    nh = 0 if dheads is None else dheads.shape[-1]
    if wgrad_dheads is None:
        wgrad_dheads = dheads          # head-weight gradient wanted whenever dheads drives the backward
    nhw = 0 if wgrad_dheads is None else wgrad_dheads.shape[-1]
    if wgrad_dheads is not None and dw_head is None:
        dw_head = torch.empty(nhw, H, dtype=F32, device=dev)
    # the h = 256 step path forms dx = dG W_ih inside its per-step recurrent product (same dG fragments) when I == H
    dx_in_bwd = bool(need_dx and lstm_bwd_caps(x.device, I, H) & 1) or bwd_done
    if dgates_tile and (bwd_done or need_dx):
        raise RuntimeError("lstm_bwd: dgates_tile is for one uav_lstm_bwd + uav_lstm_wgrad pair without dx")
    with _tile_request(dgates, dgates_tile, N, T, I, H) as request:
        _t = None if bwd_done else KERNEL_TIMER.bracket("lstm_bwd")
        if not bwd_done:
            check(lib().uav_lstm_bwd(_h(x), _p(keep, F32, (N, T), "keep"), _p(stash, F32, (N, T, 6 * H), "stash"),
                                     _p(w_hh, F32, (4 * H, H), "w_hh"), _p(dy, F32, (N, T, H), "dy"),
                                     _p(dheads, F32, (N, T, nh), "dheads"), _p(w_head, F32, (nh, H), "w_head"), nh,
                                     _p(dhn, F32, (N, H), "dhn"), _p(dcn, F32, (N, H), "dcn"), N, T, H,
                                     _pdg(dgates, N, T, H), _p(dh0), _p(dc0),
                                     _p(w_ih, F32, (4 * H, I), "w_ih") if dx_in_bwd else None, I, _p(dx) if dx_in_bwd else None,
                                     _stream()), "uav_lstm_bwd")
        request.written = True
        if _t is not None:
            _t.record()
        _t = KERNEL_TIMER.bracket("lstm_wgrad")
        check(lib().uav_lstm_wgrad(_h(x), _p(x, F32, (N, T, I), "x"), _p(keep, F32, (N, T), "keep"), _p(h0, F32, (N, H), "h0"),
                                   _p(y, F32, (N, T, H), "y"), _p(stash, F32, (N, T, 6 * H), "stash"),
                                   _pdg(dgates, N, T, H), _p(w_ih, F32, (4 * H, I), "w_ih"),
                                   _p(wgrad_dheads, F32, (N, T, nhw), "dheads"), nhw, N, T, I, H,
                                   _p(dw_ih, F32, (4 * H, I), "dw_ih"), _p(dw_hh, F32, (4 * H, H), "dw_hh"),
                                   _p(db, F32, (4 * H,), "db"), _p(db_hh, F32, (4 * H,), "db_hh"), _p(dw_head, F32, (nhw, H), "dw_head"),
                                   None if dx_in_bwd else _p(dx), _stream()),
              "uav_lstm_wgrad")
        if _t is not None:
            _t.record()
    return {"dx": dx, "dw_ih": dw_ih, "dw_hh": dw_hh, "db": db, "dh0": dh0, "dc0": dc0, "dgates": dgates,
            "dw_head": dw_head}


def env_materialise(state, n_env, cfg, env_index, out=None):
    out = torch.empty(500, 500, 2, dtype=F64, device=state.device) if out is None else out
    check(lib().uav_env_materialise(_h(state), _p(state, U8, name="env state"), n_env, C.byref(cfg), int(env_index),
                                    _p(out, F64, (500, 500, 2), "field_out"), _stream()), "uav_env_materialise")
    return out


def ln_relu(z, gamma, beta, want_stats=False):
    """relu(LayerNorm(z)) over the rows of z [rows, cols]; z is overwritten with the normalised values.
    want_stats: also return rstd [rows] (with z = xhat, what ln_relu_bwd needs)."""
    rows, cols = z.shape
    a = torch.empty_like(z)
    rstd = torch.empty(rows, dtype=F32, device=z.device)
    check(lib().uav_ln_relu(_h(z), _p(z, F32, (rows, cols), "z"), _p(a, F32), _p(rstd, F32), _p(gamma, F32, (cols,), "gamma"),
                            _p(beta, F32, (cols,), "beta"), rows, cols, _stream()), "uav_ln_relu")
    return (a, rstd) if want_stats else a


def ln_relu_bwd(d, xhat, rstd, gamma, beta, dgamma=None, dbeta=None):
    """d [rows, cols] = dL/da on entry, dL/dz on return (in place); returns (d, dgamma, dbeta), both [cols], overwritten."""
    rows, cols = d.shape
    dg = torch.empty(cols, dtype=F32, device=d.device) if dgamma is None else dgamma
    db = torch.empty(cols, dtype=F32, device=d.device) if dbeta is None else dbeta
    check(lib().uav_ln_relu_bwd(_h(d), _p(d, F32, (rows, cols), "d"), _p(xhat, F32, (rows, cols), "xhat"),
                                _p(rstd, F32, (rows,), "rstd"), _p(gamma, F32, (cols,), "gamma"), _p(beta, F32, (cols,), "beta"),
                                rows, cols, _p(dg, F32, (cols,), "dgamma"), _p(db, F32, (cols,), "dbeta"), _stream()),
          "uav_ln_relu_bwd")
    return d, dg, db


def smooth_l1(pred, target, beta):
    """nn.SmoothL1Loss(beta) (mean) forward + backward: returns (loss f64[1] device tensor, dpred [n])."""
    n = pred.numel()
    loss = torch.zeros(1, dtype=F64, device=pred.device)
    dpred = torch.empty(n, dtype=F32, device=pred.device)
    check(lib().uav_smooth_l1(_h(pred), _p(pred, F32, (n,), "pred"), _p(target, F32, (n,), "target"), n, float(beta),
                              _p(loss, F64), _p(dpred, F32), _stream()), "uav_smooth_l1")
    return loss, dpred


def mse_bce(out, target):
    """MSE on column 0 + BCE(sigmoid(column 1)) (PPOV2.1/train_lstm.py:110-113): returns (loss f64[1], dout [n, 2])."""
    n = out.shape[0]
    loss = torch.zeros(1, dtype=F64, device=out.device)
    dout = torch.empty(n, 2, dtype=F32, device=out.device)
    check(lib().uav_mse_bce(_h(out), _p(out, F32, (n, 2), "out"), _p(target, F32, (n, 2), "target"), n, _p(loss, F64),
                            _p(dout, F32), _stream()), "uav_mse_bce")
    return loss, dout


def clip_adamw(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=1.0,
               gnorm_out=None):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW step on flat buffers (train_lstm.py:67,91-92)."""
    n = param.numel()
    check(lib().uav_clip_adamw(_h(param), _p(param, F32, (n,), "param"), _p(grad, F32, (n,), "grad"),
                               _p(exp_avg, F32, (n,), "exp_avg"), _p(exp_avg_sq, F32, (n,), "exp_avg_sq"), n, int(step),
                               float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm),
                               _p(gnorm_out, F32, (1,), "gnorm_out"), _stream()), "uav_clip_adamw")


def colsum(x, out=None):
    rows, cols = x.shape
    out = torch.empty(cols, dtype=F32, device=x.device) if out is None else out
    check(lib().uav_colsum(_h(x), _p(x, F32, (rows, cols), "x"), rows, cols, _p(out, F32, (cols,), "out"), _stream()),
          "uav_colsum")
    return out


# ----------------------------------------------------------------------------- R1
def rollout_lstm(env_state, n_env, cfg, params, hidden, horizon, it, cur_obs, h, c, bufs, last_val=None,
                 forced_act=None, noise=None, nan_count=None, stash=None, y=None, info=None, heads=None):
    """Fused persistent rollout (csrc/rollout.hip).  bufs: dict obs[N,T,D] act rew val logp done flags keep, with
    D = 6 + cfg.trend_k observation features (cur_obs [N,D]; params laid out for an input width of D)."""
    N, T, D = n_env, horizon, 6 + cfg.trend_k
    _t = KERNEL_TIMER.bracket("rollout")
    check(lib().uav_rollout(_h(cur_obs), _p(env_state, U8, name="env state"), N, C.byref(cfg), 1,
                            _p(params, F32, name="params"), int(hidden), T, int(it),
                            _p(cur_obs, F32, (N, D), "cur_obs"), _p(h, F32, (N, hidden), "h"), _p(c, F32, (N, hidden), "c"),
                            _p(bufs["obs"], F32, (N, T, D), "obs"), _p(bufs["act"], I32, (N, T), "act"),
                            _p(bufs["rew"], F32, (N, T), "rew"), _p(bufs["val"], F32, (N, T), "val"),
                            _p(bufs["logp"], F32, (N, T), "logp"), _p(bufs["done"], F32, (N, T), "done"),
                            _p(bufs["flags"], U8, (N, T), "flags"), _p(bufs["keep"], F32, (N, T), "keep"),
                            _p(last_val, F32, (N,), "last_val"), _p(forced_act, I32, (N, T), "forced_act"),
                            _p(noise, F64, (N, T, 2), "noise"), _p(nan_count, I32, (1,), "nan_count"),
                            _p(stash, F32, (N, T, 6 * hidden), "stash"), _p(y, F32, (N, T, hidden), "y"),
                            _p(info, F32, (N, T, 10), "info"), _p(heads, F32, (N, T, 6), "heads"), _stream()),
          "uav_rollout")
    if _t is not None:
        _t.record()


def rollout_mlp(env_state, n_env, cfg, params, horizon, it, cur_obs, bufs, last_val=None, forced_act=None, noise=None,
                nan_count=None, info=None, heads=None, trend=False):
    """Fused persistent rollout of the reference's MLP policy (csrc/mlp_rollout.hip): uav_rollout with policy_kind 0.
    trend=True: policy_kind 2, the MLP with D = 6 + cfg.trend_k inputs (cur_obs [N,D], obs [N,T,D], params of
    mlp_param_count(D) floats); with cfg.trend_k = 0 that is kind 0's kernel and bits."""
    N, T, D = n_env, horizon, 6 + (cfg.trend_k if trend else 0)
    if trend:
        _mlp_trend_params("rollout_mlp", params, cfg.trend_k)
    _t = KERNEL_TIMER.bracket("rollout")
    check(lib().uav_rollout(_h(cur_obs), _p(env_state, U8, name="env state"), N, C.byref(cfg), 2 if trend else 0,
                            _p(params, F32, name="params"), 0, T, int(it), _p(cur_obs, F32, (N, D), "cur_obs"), None, None,
                            _p(bufs["obs"], F32, (N, T, D), "obs"), _p(bufs["act"], I32, (N, T), "act"),
                            _p(bufs["rew"], F32, (N, T), "rew"), _p(bufs["val"], F32, (N, T), "val"),
                            _p(bufs["logp"], F32, (N, T), "logp"), _p(bufs["done"], F32, (N, T), "done"),
                            _p(bufs["flags"], U8, (N, T), "flags"), None, _p(last_val, F32, (N,), "last_val"),
                            _p(forced_act, I32, (N, T), "forced_act"), _p(noise, F64, (N, T, 2), "noise"),
                            _p(nan_count, I32, (1,), "nan_count"), None, None, _p(info, F32, (N, T, 10), "info"),
                            _p(heads, F32, (N, T, 6), "heads"), _stream()), "uav_rollout")
    if _t is not None:
        _t.record()


def greedy_recs(n_env, steps, obs_dim, device):
    """The record tensors of one greedy launch: act i32 [N,steps], obs [N,steps,obs_dim], pos [N,steps,2], flags u8 [N,steps]."""
    N, k = n_env, steps
    return {"act": torch.empty(N, k, dtype=I32, device=device), "obs": torch.empty(N, k, obs_dim, dtype=F32, device=device),
            "pos": torch.empty(N, k, 2, dtype=F32, device=device), "flags": torch.empty(N, k, dtype=U8, device=device)}


def _greedy(env_state, n_env, cfg, params, hidden, steps, cur_obs, h, c, active, recs, noise, nan_count, rule=None, stop_win=None,
            stop_cnt=None, rule_val=None, trend=False):
    """uav_greedy_episodes, or with a `rule` uav_greedy_episodes_stop: the same arguments with the rule's four behind them."""
    N, T, D = n_env, steps, 6 + cfg.trend_k
    kind = (2 if trend else 0) if hidden == 0 else 1
    if kind == 2:
        _mlp_trend_params("greedy_episodes", params, cfg.trend_k)
    if nan_count is None:
        nan_count = torch.zeros(1, dtype=I32, device=cur_obs.device)
    symbol, tail = "uav_greedy_episodes", ()
    if rule is not None:
        W = int(rule.window)
        symbol, tail = "uav_greedy_episodes_stop", (C.byref(rule), _p(stop_win, F32, (N, W, 2), "stop_win"),
                                                    _p(stop_cnt, I32, (N,), "stop_cnt"), _p(rule_val, F32, (N, T), "rule_val"))
    _t = KERNEL_TIMER.bracket("greedy")
    check(getattr(lib(), symbol)(_h(cur_obs), _p(env_state, U8, name="env state"), N, C.byref(cfg), kind,
                                 _p(params, F32, name="params"), int(hidden), T, _p(cur_obs, F32, (N, D), "cur_obs"),
                                 _p(h, F32, (N, hidden), "h") if kind else None, _p(c, F32, (N, hidden), "c") if kind else None,
                                 _p(active, U8, (N,), "active"), _p(noise, F64, (N, T, 2), "noise"),
                                 _p(recs["act"], I32, (N, T), "act"), _p(recs["obs"], F32, (N, T, D), "obs"),
                                 _p(recs["pos"], F32, (N, T, 2), "pos"), _p(recs["flags"], U8, (N, T), "flags"),
                                 _p(nan_count, I32, (1,), "nan_count"), *tail, _stream()), symbol)
    if _t is not None:
        _t.record()


def greedy_episodes(env_state, n_env, cfg, params, hidden, steps, cur_obs, h, c, active, recs, noise=None, nan_count=None,
                    trend=False):
    """`steps` steps of greedy evaluation episodes on the fused rollout kernels (uav_greedy_episodes): argmax action, no
    auto-reset, ended / inactive envs frozen.  hidden = 0 (h, c None): the reference's MLP; 64 / 128: the single-layer LSTM.
    cur_obs [N,D], h, c [N,H], active u8 [N] are in/out; recs: dict act i32 [N,steps], obs [N,steps,D], pos [N,steps,2],
    flags u8 [N,steps] (bit0 done, bit1 reached, bit2 not stepped; greedy_recs allocates it); noise f64 [N,steps,2] or None.
    D = 6 + cfg.trend_k.  The LSTM takes trend_k 0, 1 or 2; the MLP (hidden = 0) takes trend_k = 0, or with trend=True
    (policy_kind 2) an MLP of D inputs at trend_k 0, 1 or 2, params of mlp_param_count(D) floats."""
    _greedy(env_state, n_env, cfg, params, hidden, steps, cur_obs, h, c, active, recs, noise, nan_count, trend=trend)


STOP_WIN_MAX = 16


def make_stop_rule(window=10, pos_std_max=2.0, conc_coef=2.0, conc_peak=100.0, conc_min=80.0):
    """struct uav_stop_rule; the defaults are PPOV1.1/evaluate_model.py's (window 10, std below 2.0 px, CONC_REWARD_COEF 2.0,
    CONC_PEAK 100.0, threshold 0.8 * CONC_PEAK).  pos_std_max = 0 never fires."""
    if not 1 <= int(window) <= STOP_WIN_MAX:
        raise RuntimeError(f"stop rule: window {window} outside 1 .. {STOP_WIN_MAX}")
    return _lib.StopRule(int(window), float(pos_std_max), float(conc_coef), float(conc_peak), float(conc_min))


def greedy_episodes_stop(env_state, n_env, cfg, params, hidden, steps, cur_obs, h, c, active, recs, rule, stop_win, stop_cnt,
                         noise=None, nan_count=None, rule_val=None, trend=False):
    """greedy_episodes with evaluate_model.py's stop rule applied on the device after every step (uav_greedy_episodes_stop):
    a hit ends the env's episode as `done` does and sets flags bit3 in the step's record.  rule: make_stop_rule(...);
    stop_win f32 [N, window, 2] (the env's last positions, oldest first) and stop_cnt i32 [N] (valid rows) are in/out and
    carry the window across calls (zeros start an episode); rule_val: optional f32 [N, steps], pos_std of every stepped step
    with a full window, NaN otherwise.  trend: as greedy_episodes."""
    _greedy(env_state, n_env, cfg, params, hidden, steps, cur_obs, h, c, active, recs, noise, nan_count, rule, stop_win, stop_cnt,
            rule_val, trend=trend)


def greedy_tail(env_state, cfg, y, w_head, b_head, t, cur_obs, active, recs, nan_count, noise=None, rule=None, stop_win=None,
                stop_cnt=None, rule_val=None):
    """uav_greedy_tail: everything of greedy evaluation step t after the recurrent layers in one launch -- the logits of y (the top
    layer's output, [N, H] or [N, 1, H]; rows may be strided), argmax, the environment step without auto-reset, the stop rule
    when `rule` (make_stop_rule) is given, and column t of recs (greedy_recs: act / obs / pos / flags [N, steps, ..]) and of
    rule_val [N, steps].  w_head [A + 1, H] / b_head [A + 1] are the policy's head rows (the critic row is not read).  cur_obs
    [N, D], active u8 [N], stop_win / stop_cnt are in/out; noise f64 [N, 2] or None.  Inactive envs get the "not stepped" record
    and are otherwise left alone.  Identical results to gemm_rows + argmax + env_step (+ stop_stability) on envs that run."""
    N, H = y.shape[0], y.shape[-1]
    D = 6 + cfg.trend_k
    T = recs["act"].shape[1]
    if not y.is_cuda or y.dtype != F32 or y.numel() != N * H or y.stride(-1) != 1:
        raise RuntimeError(f"y: expected a GPU float32 [N, H] or [N, 1, H] tensor with contiguous rows, got {tuple(y.shape)} {y.dtype}")
    A1 = w_head.shape[0]
    tail = (None, None, None, None)
    if rule is not None:
        W = int(rule.window)
        tail = (C.byref(rule), _p(stop_win, F32, (N, W, 2), "stop_win"), _p(stop_cnt, I32, (N,), "stop_cnt"),
                _p(rule_val, F32, (N, T), "rule_val"))
    elif rule_val is not None:
        raise RuntimeError("rule_val belongs to a rule")
    check(lib().uav_greedy_tail(_h(y), _p(env_state, U8, name="env state"), N, C.byref(cfg), C.c_void_p(y.data_ptr()),
                                int(y.stride(0)) if N > 1 else H, H, _p(w_head, F32, (A1, H), "w_head"),
                                _p(b_head, F32, (A1,), "b_head"), A1 - 1, T, int(t), _p(noise, F64, (N, 2), "noise"),
                                _p(cur_obs, F32, (N, D), "cur_obs"), _p(active, U8, (N,), "active"),
                                _p(recs["act"], I32, (N, T), "act"), _p(recs["obs"], F32, (N, T, D), "obs"),
                                _p(recs["pos"], F32, (N, T, 2), "pos"), _p(recs["flags"], U8, (N, T), "flags"),
                                _p(nan_count, I32, (1,), "nan_count"), *tail, _stream()), "uav_greedy_tail")


EVAL_SUM_N = 8             # UAV_EVAL_SUM_N
# the eight sums of uav_greedy_summary, include/uavppo.h UAV_EVAL_SUM_*
EVAL_SUM_NAMES = ("episodes", "successes", "steps", "dev", "dev_sq", "dev_success", "cut_off", "nan")
BEST_N = 7                 # UAV_BEST_N
# the seven slots of uav_keep_best's state, include/uavppo.h UAV_BEST_*
BEST_NAMES = ("successes", "steps", "iteration", "seen", "improved", "skipped", "took")


def greedy_reduce(recs, t0, ep_steps, ep_state, ep_pos):
    """E1 (uav_greedy_reduce): the records of one chunk (greedy_recs: flags [N, k], obs [N, k, D], pos [N, k, 2]) after t0 earlier
    steps -> ep_steps i32 [N], ep_state u8 [N] (bit0 ended, bit1 by the rule), ep_pos f64 [N, 2], in place (eval_track.reduce_chunk).
    No host sync."""
    N, k, D = recs["obs"].shape
    check(lib().uav_greedy_reduce(_h(ep_pos), _p(recs["flags"], U8, (N, k), "flags"), _p(recs["obs"], F32, (N, k, D), "obs"),
                                  _p(recs["pos"], F32, (N, k, 2), "pos"), N, k, D, int(t0), _p(ep_steps, I32, (N,), "ep_steps"),
                                  _p(ep_state, U8, (N,), "ep_state"), _p(ep_pos, F64, (N, 2), "ep_pos"), _stream()), "uav_greedy_reduce")


def greedy_summary(ep_steps, ep_state, ep_pos, src, limit, success_distance, sums, nan_count=None, deviation=None, steps=None,
                   success=None):
    """E2 (uav_greedy_summary): sums f64 [EVAL_SUM_N] of an evaluation whose episodes stand as ep_* say, against the sources src
    f64 [N, 2] (eval_track.summarise, its order of summation); optional per-env outputs deviation f64 [N], steps i32 [N], success
    u8 [N]; nan_count i32 [1] or None -> sums[7].  No host sync."""
    N = ep_steps.numel()
    check(lib().uav_greedy_summary(_h(sums), _p(ep_steps, I32, (N,), "ep_steps"), _p(ep_state, U8, (N,), "ep_state"),
                                   _p(ep_pos, F64, (N, 2), "ep_pos"), _p(src, F64, (N, 2), "src"), N, int(limit), float(success_distance),
                                   _p(nan_count, I32, (1,), "nan_count"), _p(deviation, F64, (N,), "deviation"),
                                   _p(steps, I32, (N,), "steps"), _p(success, U8, (N,), "success"),
                                   _p(sums, F64, (EVAL_SUM_N,), "sums"), _stream()), "uav_greedy_summary")
    return sums


def keep_best(state, sums, iteration, cand, best):
    """E3 (uav_keep_best): the decision of eval_track.better_rule on state f64 [BEST_N] (zeros = fresh) from the all-reduced sums,
    and best[:] = cand[:] under it (f32, the same number of elements).  Two launches, no host sync."""
    n = cand.numel()
    if best.numel() != n:
        raise RuntimeError(f"keep_best: best has {best.numel()} elements, cand has {n}")
    check(lib().uav_keep_best(_h(state), _p(state, F64, (BEST_N,), "state"), _p(sums, F64, (EVAL_SUM_N,), "sums"), int(iteration),
                              _p(cand, F32, name="cand"), _p(best, F32, name="best"), n, _stream()), "uav_keep_best")


SRC_STATE_N, SRC_EST_N, SRC_SUM_N = 20, 8, 12      # UAV_SRC_STATE_N, UAV_SRC_EST_N, UAV_SRC_SUM_N
# uav_source_solve's status codes and the twelve sums of uav_source_summary, include/uavppo.h UAV_SRC_*
SRC_STATUS_NAMES = ("fitted", "few", "degenerate", "not_a_peak")
SRC_SUM_NAMES = ("envs", "fitted", "few", "degenerate", "not_a_peak", "err", "err_sq", "within", "sigma_rel", "peak_rel", "max_err",
                 "max_envs")


def source_fit_cfg(use_tke=True, min_samples=5, background=0.0, floor=1.0, min_pivot=1e-6, **_):
    """struct uav_source_fit_cfg from source_fit.check_source_fit's dict (keys that are not the struct's are ignored)."""
    return _lib.SourceFitCfg(int(bool(use_tke)), int(min_samples), float(background), float(floor), float(min_pivot))


def _source_moments(entry, state_n, recs, cfg, state, ended):
    """uav_source_moments / uav_source_moments6: one argument list, the state's width apart"""
    N, k, D = recs["obs"].shape
    check(getattr(lib(), entry)(_h(state), _p(recs["flags"], U8, (N, k), "flags"), _p(recs["obs"], F32, (N, k, D), "obs"),
                                _p(recs["pos"], F32, (N, k, 2), "pos"), N, k, D, C.byref(cfg), _p(ended, U8, (N,), "ended"),
                                _p(state, F64, (N, state_n), "state"), _stream()), entry)


def _source_solve(entry, state_n, est_n, state, cfg, est, status):
    """uav_source_solve / uav_source_solve6: one argument list, the widths of state and est apart"""
    N = state.shape[0]
    check(getattr(lib(), entry)(_h(state), _p(state, F64, (N, state_n), "state"), N, C.byref(cfg), _p(est, F64, (N, est_n), "est"),
                                _p(status, U8, (N,), "status"), _stream()), entry)


def source_moments(recs, cfg, state, ended=None):
    """S1 (uav_source_moments): the records of one chunk (greedy_recs: flags [N, k], obs [N, k, D], pos [N, k, 2]) added to state f64
    [N, SRC_STATE_N] in place (source_fit.moments_chunk); ended u8 [N] or None: envs left alone.  No host sync."""
    _source_moments("uav_source_moments", SRC_STATE_N, recs, cfg, state, ended)


def source_solve(state, cfg, est, status):
    """S2 (uav_source_solve): state f64 [N, SRC_STATE_N] -> est f64 [N, SRC_EST_N], status u8 [N] (source_fit.solve).  No host sync."""
    _source_solve("uav_source_solve", SRC_STATE_N, SRC_EST_N, state, cfg, est, status)


def source_summary(est, status, src, sigma_true, peak_true, loc_tol, sums, loc_err=None):
    """S3 (uav_source_summary): sums f64 [SRC_SUM_N] of the estimates against the sources src f64 [N, 2] (source_fit.summarise, its
    order of summation); loc_err f64 [N] or None takes each fitted env's error.  No host sync."""
    N = status.numel()
    check(lib().uav_source_summary(_h(sums), _p(est, F64, (N, SRC_EST_N), "est"), _p(status, U8, (N,), "status"),
                                   _p(src, F64, (N, 2), "src"), N, float(sigma_true), float(peak_true), float(loc_tol),
                                   _p(loc_err, F64, (N,), "loc_err"), _p(sums, F64, (SRC_SUM_N,), "sums"), _stream()),
          "uav_source_summary")
    return sums


PLUME_PARAM_N, SRC6_STATE_N, SRC6_EST_N, SRC6_SUM_N = 8, 33, 10, 16      # UAV_PLUME_PARAM_N, UAV_SRC6_STATE_N, _EST_N, _SUM_N
# the sixteen sums of uav_source_summary6, include/uavppo.h UAV_SRC_SUM_* (the first eight) and UAV_SRC6_SUM_*
SRC6_SUM_NAMES = ("envs", "fitted", "few", "degenerate", "not_a_peak", "err", "err_sq", "within", "sigma_major_rel", "sigma_minor_rel",
                  "theta_err", "peak_rel", "strength_rel", "max_err", "max_envs", "truth_envs")


def plume_bank(params, seed, index0=0, out=None, device="cuda"):
    """P1 (uav_plume_bank): bank f64 [F, 500, 500, 2] of elliptical-Gaussian plumes with E3's turbulence of the global envs index0 ..
    index0 + F - 1 at episode 0 under `seed`.  params: HOST f64 [F, PLUME_PARAM_N] (numpy; source_aniso.plume_params builds it).  No
    host sync."""
    import numpy as np
    prm = np.ascontiguousarray(np.asarray(params, np.float64))
    if prm.ndim != 2 or prm.shape[1] != PLUME_PARAM_N:
        raise RuntimeError(f"params: expected shape (F, {PLUME_PARAM_N}), got {prm.shape}")
    F = prm.shape[0]
    if out is None:
        out = torch.empty(F, 500, 500, 2, dtype=F64, device=device)
    check(lib().uav_plume_bank(_h(out), prm.ctypes.data_as(C.c_void_p), F, int(seed) & 0xFFFFFFFFFFFFFFFF, int(index0),
                               _p(out, F64, (F, 500, 500, 2), "bank"), _stream()), "uav_plume_bank")
    return out


def source_moments6(recs, cfg, state, ended=None):
    """A1 (uav_source_moments6): source_moments with six basis functions: state f64 [N, SRC6_STATE_N] in place
    (source_aniso.moments_chunk6).  No host sync."""
    _source_moments("uav_source_moments6", SRC6_STATE_N, recs, cfg, state, ended)


def source_solve6(state, cfg, est, status):
    """A2 (uav_source_solve6): state f64 [N, SRC6_STATE_N] -> est f64 [N, SRC6_EST_N], status u8 [N] (source_aniso.solve6).  No host
    sync."""
    _source_solve("uav_source_solve6", SRC6_STATE_N, SRC6_EST_N, state, cfg, est, status)


def source_summary6(est, status, src, truth, loc_tol, sums, loc_err=None):
    """A3 (uav_source_summary6): sums f64 [SRC6_SUM_N] of the estimates against the sources src f64 [N, 2] and the per-env truth f64
    [N, 4] = {sigma_major, sigma_minor, theta, peak} or None (source_aniso.summarise6, its order of summation).  No host sync."""
    N = status.numel()
    check(lib().uav_source_summary6(_h(sums), _p(est, F64, (N, SRC6_EST_N), "est"), _p(status, U8, (N,), "status"),
                                    _p(src, F64, (N, 2), "src"), _p(truth, F64, (N, 4), "truth"), N, float(loc_tol),
                                    _p(loc_err, F64, (N,), "loc_err"), _p(sums, F64, (SRC6_SUM_N,), "sums"), _stream()),
          "uav_source_summary6")
    return sums


SRC_STOP_STATE_N = 27      # UAV_SRC_STOP_STATE_N
# the fields of uav_source_stop_scan's state behind the 17 accumulators, include/uavppo.h UAV_SRC_STOP_*
SRC_STOP_PREV_X, SRC_STOP_PREV_Y, SRC_STOP_PREV_FITTED, SRC_STOP_RUN, SRC_STOP_HIT_STEP, SRC_STOP_EST = 17, 18, 19, 20, 21, 22


def source_stop_cfg(settle_tol=0.5, patience=3, near=float("inf"), min_steps=0):
    """struct uav_source_stop_cfg from source_stop.check_source_stop's dict."""
    return _lib.SourceStopCfg(float(settle_tol), float(near), int(patience), int(min_steps))


def source_stop_scan(recs, t0, cfg, stop, state, first_hit, ended=None, active=None, mu_steps=None, status_steps=None, mark=True):
    """S4 (uav_source_stop_scan): the estimator as a stop rule over the records of one chunk (greedy_recs: flags [N, k], obs
    [N, k, D], pos [N, k, 2]) after t0 earlier steps (source_stop.stop_scan_chunk): state f64 [N, SRC_STOP_STATE_N] in place,
    first_hit i32 [N] (-1: none); mark: the flags are rewritten in place (bit3 on the hit, bit2 behind it) and active u8 [N] (or
    None) cleared at the hits; optional mu_steps f64 [N, k, 2], status_steps u8 [N, k].  No host sync."""
    N, k, D = recs["obs"].shape
    check(lib().uav_source_stop_scan(_h(state), _p(recs["flags"], U8, (N, k), "flags"), _p(recs["obs"], F32, (N, k, D), "obs"),
                                     _p(recs["pos"], F32, (N, k, 2), "pos"), N, k, D, int(t0), C.byref(cfg), C.byref(stop),
                                     _p(ended, U8, (N,), "ended"), _p(active, U8, (N,), "active"),
                                     _p(state, F64, (N, SRC_STOP_STATE_N), "state"), _p(first_hit, I32, (N,), "first_hit"),
                                     _p(mu_steps, F64, (N, k, 2), "mu_steps"), _p(status_steps, U8, (N, k), "status_steps"),
                                     int(bool(mark)), _stream()), "uav_source_stop_scan")
    return first_hit


def stop_stability(rule, pos, obs2, stop_win, stop_cnt, active=None, stop=None, value=None):
    """One step of the stop rule for envs stepped by other means (uav_stop_stability): pos f32 [N, 2] (agent_pos after the
    move), obs2 f32 [N] or a column view such as obs[:, 2] (any element stride), active u8 [N] or None (all).  Updates
    stop_win [N, window, 2] / stop_cnt [N]; returns (stop u8 [N], value f32 [N]: pos_std, NaN while the window is not full).
    Inactive envs: stop 0, value NaN, window untouched."""
    N, W = pos.shape[0], int(rule.window)
    if obs2.dim() != 1 or obs2.shape[0] != N or obs2.dtype != F32 or not obs2.is_cuda:
        raise RuntimeError(f"obs2: expected a GPU float32 vector of {N} elements, got {tuple(obs2.shape)} {obs2.dtype}")
    if stop is None:
        stop = torch.empty(N, dtype=U8, device=pos.device)
    if value is None:
        value = torch.empty(N, dtype=F32, device=pos.device)
    check(lib().uav_stop_stability(_h(pos), N, C.byref(rule), _p(pos, F32, (N, 2), "pos"), C.c_void_p(obs2.data_ptr()),
                                   int(obs2.stride(0)) if N > 1 else 1, _p(active, U8, (N,), "active"),
                                   _p(stop_win, F32, (N, W, 2), "stop_win"), _p(stop_cnt, I32, (N,), "stop_cnt"),
                                   _p(stop, U8, (N,), "stop"), _p(value, F32, (N,), "value"), _stream()), "uav_stop_stability")
    return stop, value


# ----------------------------------------------------------------------------- GAIL discriminator (csrc/disc.hip)
DISC_HIDDEN = 128


def disc_param_count(obs_dim, n_act, hidden=DISC_HIDDEN):
    n = int(lib().uav_disc_param_count(int(obs_dim), int(n_act), int(hidden)))
    if n == 0:
        raise RuntimeError(f"uav_disc_param_count failed: {lib().uav_last_error().decode()}")
    return n


def disc_grad(params, obs_e, act_e, obs_p, act_p, n_act, inv_ne=None, inv_np=None, loss_sums=None, grad=None, ctx=None):
    """Forward + two BCE means + backward of the discriminator over the expert rows (obs_e [n_e, obs_dim], act_e i32 [n_e],
    label 1) and the policy rows (label 0) in one pass (uav_disc_grad).  inv_ne / inv_np default to 1 / n_e, 1 / n_p (ranks pass
    1 / the global counts).  Returns (loss_sums f64[4]: expert sum, policy sum, correct rows, NaN / bad-action rows; grad
    [param_count]).  ctx: a uav_ctx handle of the tensors' device to run on instead of the device's shared one."""
    n_e, n_p = int(obs_e.shape[0]), int(obs_p.shape[0])
    od = int(obs_p.shape[1]) if n_p else int(obs_e.shape[1])
    P = disc_param_count(od, n_act)
    loss_sums = torch.empty(4, dtype=F64, device=params.device) if loss_sums is None else loss_sums
    grad = torch.empty(P, dtype=F32, device=params.device) if grad is None else grad
    inv_ne = (1.0 / n_e if n_e else 0.0) if inv_ne is None else inv_ne
    inv_np = (1.0 / n_p if n_p else 0.0) if inv_np is None else inv_np
    _t = KERNEL_TIMER.bracket("disc_grad")
    check(lib().uav_disc_grad(_h(params) if ctx is None else ctx, _p(params, F32, (P,), "params"),
                              _p(obs_e, F32, (n_e, od), "obs_e") if n_e else None, _p(act_e, I32, (n_e,), "act_e") if n_e else None, n_e,
                              _p(obs_p, F32, (n_p, od), "obs_p") if n_p else None, _p(act_p, I32, (n_p,), "act_p") if n_p else None, n_p,
                              od, int(n_act), DISC_HIDDEN, float(inv_ne), float(inv_np), _p(loss_sums, F64, (4,), "loss_sums"),
                              _p(grad, F32, (P,), "grad"), _stream()), "uav_disc_grad")
    if _t is not None:
        _t.record()
    return loss_sums, grad


def disc_reward(params, obs, act, n_act, gail_coef=1.0, env_coef=1.0, rew_env=None, out=None):
    """out[i] = env_coef * rew_env[i] + gail_coef * softplus(z_i) over the rows obs [n, obs_dim], act i32 [n] (uav_disc_reward);
    rew_env None = 0; out may be rew_env itself."""
    n, od = int(obs.shape[0]), int(obs.shape[1])
    P = disc_param_count(od, n_act)
    out = torch.empty(n, dtype=F32, device=obs.device) if out is None else out
    _t = KERNEL_TIMER.bracket("disc_reward")
    check(lib().uav_disc_reward(_h(params), _p(params, F32, (P,), "params"), _p(obs, F32, (n, od), "obs"), _p(act, I32, (n,), "act"), n,
                                od, int(n_act), DISC_HIDDEN, float(env_coef), float(gail_coef), _p(rew_env, F32, (n,), "rew_env"),
                                _p(out, F32, (n,), "rew_out"), _stream()), "uav_disc_reward")
    if _t is not None:
        _t.record()
    return out


# ----------------------------------------------------------------------------- PPOV2.1 peak-and-stop rule (csrc/peak_stop.hip)
def peak_stop_param_count(hidden=32):
    n = int(lib().uav_peak_stop_param_count(int(hidden)))
    if n == 0:
        raise RuntimeError(f"uav_peak_stop_param_count failed: {lib().uav_last_error().decode()}")
    return n


def _series_hist(series, hist, cnt, window, cnt_name):
    """(N, steps, window, hist pointer) of a rule call's `series` view and its [N, window - 1] history; `cnt` is the envs' i32 counter."""
    if series.dim() != 2 or series.dtype != F32 or not series.is_cuda:
        raise RuntimeError(f"series: expected a 2-D GPU float32 tensor (view), got {tuple(series.shape)} {series.dtype}")
    N, W = int(series.shape[0]), int(window)
    hist_p = _p(hist, F32, (N, max(W - 1, 0)), "hist")
    if W == 1:          # an [N, 0] tensor has no storage, the C ABI refuses a NULL hist: any valid pointer serves, none of it is touched
        hist_p = _p(cnt, I32, (N,), cnt_name)
    return N, int(series.shape[1]), W, hist_p


def peak_stop_scan(params, hidden, window, series, hist, hist_cnt, active=None, prob_min=0.8, want_values=True):
    """The PeakAndStopPredictor over every sliding window of a chunk (uav_peak_stop_scan).  params: the flat buffer of
    PeakAndStopPredictor.flat_params(); series: f32 [N, steps] view of any strides (recs["obs"][:, :, 2] as it is): env e's LSTM
    input at chunk step i; hist f32 [N, window - 1] / hist_cnt i32 [N]: the envs' last inputs, in / out (zero hist_cnt starts an
    episode); active u8 [N] or None (all).  Returns (first_hit i32 [N]: first step whose window is full and has stop_prob >
    prob_min, -1 if none; peak, prob f32 [N, steps], NaN where the window is not full or the env inactive -- None with
    want_values=False)."""
    N, T, W, hist_p = _series_hist(series, hist, hist_cnt, window, "hist_cnt")
    P = peak_stop_param_count(hidden)
    dev = series.device
    peak = torch.empty(N, T, dtype=F32, device=dev) if want_values else None
    prob = torch.empty(N, T, dtype=F32, device=dev) if want_values else None
    first_hit = torch.empty(N, dtype=I32, device=dev)
    _t = KERNEL_TIMER.bracket("peak_stop_scan")
    check(lib().uav_peak_stop_scan(_h(series), _p(params, F32, (P,), "params"), int(hidden), W, C.c_void_p(series.data_ptr()),
                                   int(series.stride(0)), int(series.stride(1)), N, T, _p(active, U8, (N,), "active"),
                                   hist_p, _p(hist_cnt, I32, (N,), "hist_cnt"), float(prob_min),
                                   _p(peak, F32, (N, T), "peak"), _p(prob, F32, (N, T), "prob"), _p(first_hit, I32, (N,), "first_hit"),
                                   _stream()), "uav_peak_stop_scan")
    if _t is not None:
        _t.record()
    return first_hit, peak, prob


# ----------------------------------------------------------------------------- PPOV2.0 threshold stop rule (csrc/threshold.hip)
def threshold_slots(steps, every=10):
    """S = ceil(steps / every): the predictor rows per env of a call of `steps` steps."""
    return (int(steps) + int(every) - 1) // int(every)


def threshold_windows(series, hist, step_cnt, active=None, window=10, every=10, min_steps=20, lo=0.0, scale=1.0, conc_scale=100.0):
    """The ConcentrationThresholdPredictor's inputs of a chunk (uav_threshold_windows).  series: f32 [N, steps] view of any strides
    (recs["obs"][:, :, 2] as it is); hist f32 [N, window - 1] / step_cnt i32 [N]: the envs' last inputs and the steps seen before
    this call (read only); active u8 [N] or None (all).  Returns x f32 [N, S, window], S = threshold_slots(steps, every): slot s of
    env e holds the scaled window of its update step t = (step_cnt[e] // every + s + 1) * every where the call reaches it and
    t >= max(window, min_steps), zeros otherwise."""
    N, T, W, hist_p = _series_hist(series, hist, step_cnt, window, "step_cnt")
    x = torch.empty(N, threshold_slots(T, every), W, dtype=F32, device=series.device)
    _t = KERNEL_TIMER.bracket("threshold_windows")
    check(lib().uav_threshold_windows(_h(series), C.c_void_p(series.data_ptr()), int(series.stride(0)), int(series.stride(1)), N, T,
                                      _p(active, U8, (N,), "active"), hist_p, _p(step_cnt, I32, (N,), "step_cnt"), W, int(every),
                                      int(min_steps), float(lo), float(scale), float(conc_scale), _p(x), _stream()),
          "uav_threshold_windows")
    if _t is not None:
        _t.record()
    return x


def threshold_rule(series, hist, step_cnt, pred, thr, active=None, window=10, every=10, min_steps=20, conc_scale=100.0, factor=0.95,
                   want_steps=True):
    """The PPOV2.0 rule over every step of a chunk (uav_threshold_rule).  series, hist, step_cnt, active as threshold_windows (hist
    and step_cnt are advanced here); pred f32 [N, S]: the predictor's outputs for threshold_windows' rows; thr f64 [N] in / out:
    the threshold in force, NaN = none yet.  Returns (first_hit i32 [N]: first step of the call at which the rule fires, -1 if
    none; stop u8 [N, steps]; thr_out f64 [N, steps] -- None, None with want_steps=False)."""
    N, T, W, hist_p = _series_hist(series, hist, step_cnt, window, "step_cnt")
    dev = series.device
    stop = torch.empty(N, T, dtype=U8, device=dev) if want_steps else None
    thr_out = torch.empty(N, T, dtype=F64, device=dev) if want_steps else None
    first_hit = torch.empty(N, dtype=I32, device=dev)
    _t = KERNEL_TIMER.bracket("threshold_rule")
    check(lib().uav_threshold_rule(_h(series), C.c_void_p(series.data_ptr()), int(series.stride(0)), int(series.stride(1)), N, T,
                                   _p(active, U8, (N,), "active"), hist_p, _p(step_cnt, I32, (N,), "step_cnt"), W, int(every),
                                   int(min_steps), float(conc_scale), float(factor), _p(pred, F32, (N, threshold_slots(T, every)), "pred"),
                                   _p(thr, F64, (N,), "thr"), _p(first_hit), _p(stop), _p(thr_out), _stream()), "uav_threshold_rule")
    if _t is not None:
        _t.record()
    return first_hit, stop, thr_out
