"""Materialised plume-field banks for the vectorised environments (BASELINE C4: "WRF-LES training_data.nc wind field").

A bank is `[F, 500, 500, 2]` f64 (concentration, tke) resident in HBM plus the `[F, 2]` source position of every field;
episode k of global env e uses field (e + k * N_total) mod F (csrc/env_core.h).  Four ways to get one:

* a file: `.npz` with arrays `conc` [F, 500, 500], `tke` [F, 500, 500], `source` [F, 2] (`conc` on the reference's 0..100
  scale, the tables its `_generate_plume` builds, environment.py:51-62), or a netCDF file with variables of the same names
  when the netCDF4 package is installed (it is not in this image; the reference names no schema for a field file -- its
  `training_data.nc` is a TRAJECTORY log, PPOV2.1/nc_info.txt -- so the names are this build's);
* `"synth:F"`: F fields generated on the device by the procedural sampler itself with E3's formula (`uav_env_materialise`),
  the generator bench.py's C4 configuration uses;
* `"aniso:F"` / `"aniso:F:rlo-rhi"`: F fields of plumes stretched along an axis, generated on the device (`uav_plume_bank`), with
  the per-field truth {sigma_major, sigma_minor, theta, peak} (`load_with_truth`);
* arrays handed over directly.
"""
from __future__ import annotations

import numpy as np
import torch

GRID = 500


def _check(conc, tke, source):
    conc, tke, source = (np.asarray(a, dtype=np.float64) for a in (conc, tke, source))
    if conc.ndim != 3 or conc.shape[1:] != (GRID, GRID) or tke.shape != conc.shape:
        raise ValueError(f"field bank: conc / tke must be [F, {GRID}, {GRID}], got {conc.shape} / {tke.shape}")
    if source.shape != (conc.shape[0], 2):
        raise ValueError(f"field bank: source must be [F, 2], got {source.shape}")
    if not (np.isfinite(conc).all() and np.isfinite(tke).all() and np.isfinite(source).all()):
        raise ValueError("field bank: non-finite values")
    return conc, tke, source


def from_arrays(conc, tke, source, device="cuda"):
    conc, tke, source = _check(conc, tke, source)
    bank = torch.from_numpy(np.stack([conc, tke], axis=-1)).to(device).contiguous()
    return bank, torch.from_numpy(source).to(device).contiguous()


def synthesise(n_fields, variant="v2.1", device="cuda", seed=4321):
    """F fields by E3's formula from the counter RNG, entirely on the device (no host tables)."""
    from . import ops
    from .vec_env import VecMethaneEnv
    gen = VecMethaneEnv(int(n_fields), variant, device, seed=seed)
    gen.reset()
    bank = torch.stack([ops.env_materialise(gen.state, int(n_fields), gen.cfg(), f) for f in range(int(n_fields))])
    return bank, gen.peek()[1]


def synthesise_aniso(n_fields, seed=4321, sigma=(20.0, 45.0), ratio=(1.5, 3.0), peak=(100.0, 100.0), device="cuda"):
    """F fields of plumes stretched along an axis (uav_plume_bank): elliptical Gaussians with E3's turbulence, generated on the
    device.  From a numpy generator seeded with `seed`: sources U[50, 450]^2, sigma_major U[sigma], sigma_minor = sigma_major /
    U[ratio], the major axis' angle U[0, pi), peak U[peak].  Returns (bank [F, 500, 500, 2], sources [F, 2], truth f64 [F, 4] =
    {sigma_major, sigma_minor, theta, peak}), all on the device."""
    from . import ops, source_aniso as sa
    F = int(n_fields)
    for name, (lo, hi) in (("sigma", sigma), ("peak", peak)):
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"synthesise_aniso: {name}=({lo}, {hi}) must be a finite range 0 < lo <= hi")
    if not (np.isfinite(ratio[0]) and np.isfinite(ratio[1]) and 1.0 <= ratio[0] <= ratio[1]):
        raise ValueError(f"synthesise_aniso: ratio=({ratio[0]}, {ratio[1]}) must be a finite range 1 <= lo <= hi")
    if F < 1:
        raise ValueError(f"synthesise_aniso: n_fields={n_fields} must be at least 1")
    rng = np.random.default_rng(int(seed))
    src = rng.uniform(50.0, 450.0, (F, 2))
    s_major = rng.uniform(sigma[0], sigma[1], F)
    s_minor = s_major / rng.uniform(ratio[0], ratio[1], F)
    theta = rng.uniform(0.0, np.pi, F)
    pk = rng.uniform(peak[0], peak[1], F)
    params = sa.check_plume_params(sa.plume_params(src, s_major, s_minor, theta, pk))
    bank = ops.plume_bank(params, int(seed), 0, device=device)
    truth = np.stack([s_major, s_minor, theta, pk], 1)
    return bank, torch.from_numpy(src).to(device).contiguous(), torch.from_numpy(truth).to(device).contiguous()


def save_npz(path, bank, sources, truth=None):
    b = torch.as_tensor(bank).cpu().numpy()
    extra = {} if truth is None else {"truth": torch.as_tensor(truth).cpu().numpy()}
    np.savez_compressed(path, conc=b[..., 0], tke=b[..., 1], source=torch.as_tensor(sources).cpu().numpy(), **extra)


def parse_aniso(spec):
    """"aniso:F" or "aniso:F:rlo-rhi" -> (F, (rlo, rhi) or None); ValueError with the reason otherwise."""
    parts = str(spec).split(":")
    try:
        if parts[0] != "aniso" or len(parts) not in (2, 3):
            raise ValueError
        F = int(parts[1])
        ratio = None
        if len(parts) == 3:
            lo, hi = parts[2].split("-")
            ratio = (float(lo), float(hi))
            if not (np.isfinite(ratio[0]) and np.isfinite(ratio[1]) and 1.0 <= ratio[0] <= ratio[1]):
                raise ValueError
        if F < 1:
            raise ValueError
    except ValueError:
        raise ValueError(f"field bank {spec!r}: expected \"aniso:F\" or \"aniso:F:rlo-rhi\" with F >= 1 and 1 <= rlo <= rhi") from None
    return F, ratio


def load_with_truth(spec, variant="v2.1", device="cuda"):
    """load() with the per-field truth: (bank, sources, truth f64 [F, 4] = {sigma_major, sigma_minor, theta, peak} or None).
    "aniso:F" / "aniso:F:rlo-rhi": synthesise_aniso (with that axis-ratio range); an .npz may carry a `truth` array [F, 4]."""
    if isinstance(spec, str) and spec.startswith("aniso:"):
        F, ratio = parse_aniso(spec)
        return synthesise_aniso(F, device=device) if ratio is None else synthesise_aniso(F, ratio=ratio, device=device)
    if isinstance(spec, str) and spec.endswith(".npz"):
        with np.load(spec) as d:
            bank, sources = from_arrays(d["conc"], d["tke"], d["source"], device=device)
            truth = None
            if "truth" in d.files:
                t = np.asarray(d["truth"], np.float64)
                if t.shape != (bank.shape[0], 4):
                    raise ValueError(f"field bank {spec!r}: truth must be [F, 4], got {t.shape}")
                truth = torch.from_numpy(t).to(device).contiguous()
            return bank, sources, truth
    return (*load(spec, variant, device), None)


def load(spec, variant="v2.1", device="cuda"):
    """spec: None | "synth:F" | "aniso:F[:rlo-rhi]" | path (.npz, or netCDF when the package exists) | (conc, tke, source) arrays  ->  (bank, sources) or (None, None)."""
    if spec is None or spec == "":
        return None, None
    if isinstance(spec, (tuple, list)):
        return from_arrays(*spec, device=device)
    spec = str(spec)
    if spec.startswith("aniso:"):
        return load_with_truth(spec, variant, device)[:2]
    if spec.startswith("synth:"):
        return synthesise(int(spec.split(":", 1)[1]), variant, device)
    if spec.endswith(".npz"):
        with np.load(spec) as d:
            return from_arrays(d["conc"], d["tke"], d["source"], device=device)
    try:
        from netCDF4 import Dataset
    except ImportError as e:
        raise RuntimeError(f"field bank {spec!r}: netCDF4 is not installed here; convert the file to .npz (conc, tke, source)") from e
    with Dataset(spec, "r") as nc:
        return from_arrays(np.ma.filled(nc["conc"][:], np.nan), np.ma.filled(nc["tke"][:], np.nan),
                           np.ma.filled(nc["source"][:], np.nan), device=device)
