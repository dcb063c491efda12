"""Shared helpers for the golden-fixture tests (test infrastructure)."""
import json
import os

import numpy as np
import torch

from oracle import xfm_oracle as O
from xfm_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_DT = {"float32": torch.float32, "int64": torch.int64, "int32": torch.int32, "bool": torch.bool}
# every committed file stays under 1 MiB: a fixture that would be larger is stored as <name>.npz + <name>.part<i>.npz, and the
# first file's `golden_parts` entry says how many files there are
PART_BYTES = 900 * 1024


def _part_path(name, i, root=GOLDEN):
    return os.path.join(root, name + (".npz" if i == 0 else f".part{i}.npz"))


class Fixture:
    """The arrays of one fixture across its files: `z[key]`, `key in z`, `z.files` as on a single np.load'ed .npz."""

    def __init__(self, name, root=GOLDEN):
        first = np.load(_part_path(name, 0, root))
        n = int(first["golden_parts"]) if "golden_parts" in first.files else 1
        self._of = {}
        for z in [first] + [np.load(_part_path(name, i, root)) for i in range(1, n)]:   # a missing part raises
            for k in z.files:
                self._of[k] = z
        self._of.pop("golden_parts", None)
        self.files = list(self._of)

    def __getitem__(self, key):
        return self._of[key][key]

    def __contains__(self, key):
        return key in self._of


def save(name, arrays, root=GOLDEN):
    """Write fixture `name` (key -> array, compressed), split into parts of at most ~PART_BYTES; returns the paths written."""
    import glob
    import io
    import zlib
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.save(buf, np.asarray(v))
        n = len(zlib.compress(buf.getvalue())) + 2 * len(k) + 160   # deflated payload + zip local / central headers
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    if len(parts) > 1:
        parts[0]["golden_parts"] = np.asarray(len(parts))
    for stale in glob.glob(os.path.join(root, glob.escape(name) + ".part*.npz")):
        os.remove(stale)
    paths = []
    for i, p in enumerate(parts):
        paths.append(_part_path(name, i, root))
        np.savez_compressed(paths[-1], **p)
    return paths


def load(name):
    z = Fixture(name)
    meta = json.loads(str(z["meta"]))
    return z, meta


def state_from_spec(spec):
    """Regenerate the formula weights for a reference state_dict spec (key -> [shape, dtype])."""
    ref = {}
    for k, (shape, dt) in spec.items():
        if k.endswith("relative_position_index"):
            g = int(round((shape[0] - 1) ** 0.5))
            ref[k] = O.beit_relative_position_index(g, g)
        elif k.endswith("position_ids"):
            ref[k] = torch.arange(shape[1]).expand(1, -1).clone()
        else:
            ref[k] = torch.empty(shape, dtype=_DT[dt])
    return syn.formula_state_dict(ref)


def probe_index(n, k):
    k = min(k, n)
    if k <= 1:
        return torch.zeros(1, dtype=torch.long)
    return (torch.arange(k, dtype=torch.long) * (n - 1)) // (k - 1)


def check(z, prefix, t, atol, rtol=0.0, what=""):
    """Compare tensor `t` with the stored probe + moments of `prefix`."""
    t = t.detach().double().reshape(-1).cpu()
    n = int(z[f"{prefix}/n"])
    assert t.numel() == n, f"{prefix}: numel {t.numel()} vs golden {n}"
    ref = torch.from_numpy(z[f"{prefix}/probe"]).double()
    got = t[probe_index(n, ref.numel())]
    scale = max(float(np.sqrt(float(z[f"{prefix}/sq"]) / n)), 1e-30)
    err = float((got - ref).abs().max())
    assert err <= atol + rtol * scale, f"{what}{prefix}: max probe err {err:.3e} (rms {scale:.3e}, atol {atol}, rtol {rtol})"
    # moments: catch errors the strided probe could miss
    abs_err = abs(float(t.abs().sum()) - float(z[f"{prefix}/abs"])) / n
    assert abs_err <= atol + rtol * scale, f"{what}{prefix}: mean |.| differs by {abs_err:.3e}"
    return err


def rel_l2(z, prefix, t):
    """relative L2 error of the probed entries, and cosine on the probe"""
    t = t.detach().double().reshape(-1).cpu()
    ref = torch.from_numpy(z[f"{prefix}/probe"]).double()
    got = t[probe_index(t.numel(), ref.numel())]
    den = float(ref.norm()) + 1e-30
    cos = float((got * ref).sum() / ((got.norm() + 1e-30) * den))
    return float((got - ref).norm()) / den, cos
