"""fp64 references and elementwise error bounds of the row kernels between the GEMMs (test infrastructure; any device): the LayerNorm
family (layernorm.hip) and the cross-entropy family (cross_entropy.hip).  Poison, sentinels and the checkers are gemm_strided_util's;
poisoned_in / Outs lay a call's inputs and outputs out in such parents, and the case builders at the end are shared by the host and GPU tests.

Every reference returns (ref, b32) pairs: the fp64 value of what the kernel computes from its ACTUAL inputs, and a bound on a correct fp32
evaluation's error, one term per rounding (u32 = 2^-23 = two fp32 unit roundoffs, so a count of n u32 grants 2n roundings).  An fp32 output is
checked with check_f32(got, ref, b32), a bf16 one with check_bf16 (one more rounding of a value within b32).  A sum of n terms is charged n
roundings relative to sum |term|, whatever its order: the bounds do not encode the kernels' reduction trees.

LayerNorm forward of a row x[0..D), em = D u32 mean|x| (the sum's D adds, one multiply by 1/D):
    mean    em
    rstd    b_rstd = rstd (D/2 + 8) u32 + rstd^3 em^2
            (q = sum (x - mu)^2: D adds, a subtract and a square per term, relative to q since every term is >= 0; rsqrt halves the relative
            error and adds its own ulp; a mean off by em adds em^2 to the variance -- second order, because sum (x - mean) = 0)
    y       |w xh| b_rstd / rstd + u32 |b| + |w| rstd em      (the four roundings of (x - mu) * rstd * w + b sit in the + 8)
            = u32 ((D/2 + 8) |w xh| + |b|) + |w| rstd em, plus the rstd^3 em^2 term carried into y instead of dropped.
    POST / LS form their row in fp32 first: z = keep * scale * h + res, x' = x + (s * gamma) * h, at most three roundings:
            bz = 3 u32 (|terms|) bounds z32 / x' and, through check_bf16, the bf16 z.  The reference normalises the fp64 row, the kernel the
            fp32 one, so bz enters the bounds as an input perturbation: em += mean bz, b_rstd += rstd^3 mean(|x - mean| bz),
            y += |w| rstd bz.  (Without it the POST / LS bounds would ignore three roundings the kernel makes.)
    GELU    yg = u Phi(u), u = the y above: 1.13 b32(u) + 2^-16 |u| + u32 |yg|   (1.13 >= max |GELU'|; common.h: |delta erf| <= 2.5e-5, so Phi is
            off by <= 1.25e-5; 2^-16 = 1.53e-5 leaves the rest to the one-ulp rcp / exp2 inside the polynomial; one product)

LayerNorm backward, from the GIVEN fp32 mean / rstd (inputs of the kernel): xh = (x - mean) rstd, g = dy w, c1 = mean g, c2 = mean(g xh),
    dx = rstd (g - c1 - xh c2):
    dx      u32 rstd ((D + 8) (mean|g| + |xh| mean|g xh|) + 8 |g|)      (+ |dx0| u32 with dx_accum, + u32 |sum| for the LS stream add)
    dy = dy1 + dy2 + dy32 is formed in fp32: e_dy = (parts - 1) u32 sum |part|; with gelu_b, dy' = dy GELU'(xh w + b) carries
            e_dy' = 1.13 e_dy + 2^-16 |dy| (1 + |u|) + u32 (4 (|xh w| + |b|) |dy| + |dy'|)   (Phi and u phi off as above; u's own four roundings
            times |GELU''| < 1; the product).  An error e in dy moves dx by at most rstd (|w| e + mean(|w| e) + |xh| mean(|w| e |xh|)).
    column sums (dgamma = sum_r dy xh, dbeta = sum_r dy, dbias = sum_r dh, dls = sum_r s h dstream) follow tn_bound:
            (rows + 64) u32 sum_r |term| + sum_r (the term's own input error) + adds u32 |initial value|
            adds = 1 for the narrow kernels (one += of the folded sum), = rows for the wide kernel (one atomic add per row onto the running
            value; a single |initial| u32 would not cover them).

Cross-entropy backward, all three forms, from the GIVEN lse (and tsum for the dense form):  ref = (tsum exp(x - lse) - t) scale,
    b32 = |scale| u32 (tsum p (|x - lse| + 4) + 2 |tsum p - t|) + 2^-126
    (__expf(a) = exp2(a log2 e): the subtraction and the product each move the result by u |a| relative, = u32 |a| together; exp2's ulp,
    the product with tsum and tsum's own roundings in the label form are the + 4; the subtraction of t and the product with scale the 2;
    results under the smallest fp32 normal may flush -- the tests keep |tsum scale| <= 1, so the floor needs no factor).
    The label form's target row is evaluated in fp32 exactly as SmoothRow does (IEEE operations, no rounding left to grant).
lse forward:  u32 (|lse| + V + 90)        loss rows:  b_lse tsum + u32 (V + 8) sum |t x|"""
import math

import torch

from gemm_strided_util import (NAN, SENTINEL, U16, U32, assert_outside_untouched, check_bf16, check_f32, embed,  # noqa: F401
                               embed_vec)

F32, F64 = torch.float32, torch.float64
GELU_LIP = 1.13          # max |GELU'(u)| = 1.1290 at u = 1.41
GELU_U = 2.0 ** -16      # see the header
FLUSH = 2.0 ** -126


def _phi(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))


def _pdf(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gelu64(u):
    return u * _phi(u)


def gelu_grad64(u):
    return _phi(u) + u * _pdf(u)


def gelu_parts32(x, c3=0.7478556):
    """common.h's gelu_parts in fp32: Abramowitz-Stegun 7.1.25 -> (cdf, pdf); c3: the polynomial's leading coefficient (the host tests plant a
    wrong one)"""
    ax = x.abs()
    t = 1.0 / (0.33267 * ax + 1.0)
    e = torch.exp2(-0.72134752 * x * x)
    poly = t * (t * (t * c3 - 0.0958798) + 0.3480242)
    erf_abs = 1.0 - poly * e
    return torch.copysign(torch.full_like(x, 0.5), x) * erf_abs + 0.5, 0.39894228040143267 * e


# ------------------------------------------------------------------------------------------------------------- poisoned buffers
def poisoned_in(t, device):
    """an input as a whole-row range of a NaN-filled parent: 4 rows before and 3 after a matrix, 8 elements around a vector (offsets that
    keep the first element on a 16-byte boundary for every row length the tests use)"""
    t = t.to(device)
    return embed_vec(t, 8, 8, NAN)[0] if t.dim() == 1 else embed(t, t.shape[1], 0, 4, 3, NAN)[0]


class Outs:
    """the outputs of one call, by name: views of 7.0-filled parents, laid out like poisoned_in's"""

    def __init__(self, device):
        self.device, self.items = device, {}

    def add(self, name, shape, dtype, init=None):
        """-> the view's address; init: the output's content before the call (an accumulator), default 7.0 like its surroundings"""
        t = torch.full(shape, SENTINEL, dtype=dtype, device=self.device) if init is None else init.to(self.device).to(dtype)
        v, p = embed_vec(t, 8, 8, SENTINEL) if len(shape) == 1 else embed(t, shape[1], 0, 4, 3, SENTINEL)
        self.items[name] = (p, v, t.clone())
        return v.data_ptr()

    def __contains__(self, name):
        return name in self.items

    def __getitem__(self, name):
        return self.items[name][1]

    def check_outside(self):
        for name, (p, v, _) in self.items.items():
            assert_outside_untouched(p, v, SENTINEL, name)

    def check_unchanged(self):
        """after a rejected call: not one bit written, inside the views or outside"""
        self.check_outside()
        for name, (_, v, t0) in self.items.items():
            it = torch.int32 if v.dtype == F32 else torch.int16
            assert torch.equal(v.contiguous().view(it), t0.view(it)), f"{name} was written by a rejected call"


# ------------------------------------------------------------------------------------------------------------------ LayerNorm forward
def post_row(h, res, keep=None, drop_scale=1.0):
    """(z, bz) in fp64 for POST: z = keep * drop_scale * h + res (keep: bool mask or None)."""
    hs = h.double() * float(torch.tensor(drop_scale, dtype=F32)) if drop_scale != 1.0 else h.double()
    if keep is not None:
        hs = torch.where(keep, hs, torch.zeros_like(hs))
    r = res.double()
    return hs + r, 3 * U32 * (hs.abs() + r.abs())


def row_scale_of(row_scale, rows, rows_per_sample, device):
    """the per-row factor s of LS as an fp64 column (ones for row_scale=None)"""
    if row_scale is None:
        return torch.ones((rows, 1), dtype=F64, device=device)
    idx = torch.arange(rows, device=device) // rows_per_sample
    return row_scale.double()[idx].unsqueeze(1)


def ls_row(x, h, ls_gamma, row_scale, rows_per_sample):
    """(x', bx) in fp64 for LS: x' = x + s * gamma * h."""
    s = row_scale_of(row_scale, x.shape[0], rows_per_sample, x.device)
    t = s * ls_gamma.double() * h.double()
    return x.double() + t, 3 * U32 * (x.double().abs() + t.abs())


def ln_fwd_ref(x, w, b, eps, x_err=None, gelu=False):
    """x: the row the kernel normalises, fp64 (or exact in a narrower type); x_err: bound on |fp32 row - x| (post_row / ls_row) or None.
    Returns a dict of (ref, bound) pairs: mean, rstd ([rows]), y ([rows, D]; after the GELU when gelu)."""
    X, W, B = x.double(), w.double(), b.double()
    D = X.shape[1]
    mu = X.mean(1, keepdim=True)
    xc = X - mu
    rstd = ((xc * xc).mean(1, keepdim=True) + eps).rsqrt()
    em = D * U32 * X.abs().mean(1, keepdim=True)
    if x_err is not None:
        em = em + x_err.mean(1, keepdim=True)
    b_rstd = rstd * (D / 2 + 8) * U32 + rstd ** 3 * em * em
    if x_err is not None:
        b_rstd = b_rstd + rstd ** 3 * (xc.abs() * x_err).mean(1, keepdim=True)
    wxh = W * xc * rstd
    u = wxh + B
    b32 = wxh.abs() * (b_rstd / rstd) + U32 * B.abs() + W.abs() * rstd * em
    if x_err is not None:
        b32 = b32 + W.abs() * rstd * x_err
    y = u
    if gelu:
        y = gelu64(u)
        b32 = GELU_LIP * b32 + GELU_U * u.abs() + U32 * y.abs()
    return {"mean": (mu[:, 0], em[:, 0]), "rstd": (rstd[:, 0], b_rstd[:, 0]), "y": (y, b32)}


# ----------------------------------------------------------------------------------------------------------------- LayerNorm backward
def ln_bwd_ref(dy_parts, x, mean, rstd, w, gelu_b=None, dy_err=None):
    """dy_parts: the tensors the kernel adds up to dy (dy1, dy2, dy32; None entries skipped); x the normalised row as stored; mean / rstd the
    fp32 statistics handed to the kernel; dy_err: a bound on further roundings the caller's kernel makes on dy (the embedding's dropout
    product).  Returns a dict: dx (ref, bound), dy (the activated gradient, its error bound), xh."""
    parts = [p.double() for p in dy_parts if p is not None]
    DY = sum(parts)
    e_dy = (len(parts) - 1) * U32 * sum(p.abs() for p in parts) if len(parts) > 1 else torch.zeros_like(DY)
    if dy_err is not None:
        e_dy = e_dy + dy_err
    X, W = x.double(), w.double()
    D = X.shape[1]
    rs = rstd.double().unsqueeze(1)
    xh = (X - mean.double().unsqueeze(1)) * rs
    if gelu_b is not None:
        Bg = gelu_b.double()
        u = xh * W + Bg
        DYa = DY * gelu_grad64(u)
        e_dy = GELU_LIP * e_dy + GELU_U * DY.abs() * (1 + u.abs()) + U32 * (4 * ((xh * W).abs() + Bg.abs()) * DY.abs() + DYa.abs())
        DY = DYa
    g = DY * W
    eg = W.abs() * e_dy
    c1 = g.mean(1, keepdim=True)
    c2 = (g * xh).mean(1, keepdim=True)
    dx = rs * (g - c1 - xh * c2)
    bdx = U32 * rs * ((D + 8) * (g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) + 8 * g.abs())
    bdx = bdx + rs * (eg + eg.mean(1, keepdim=True) + xh.abs() * (eg * xh.abs()).mean(1, keepdim=True))
    return {"dx": (dx, bdx), "dy": (DY, e_dy), "xh": xh}


def colsum_bound(term, term_err=None, init=0.0, adds=1):
    """(ref, bound) of init + sum over rows of term [rows, D] (see the header)."""
    T = term.double()
    i0 = init.double() if torch.is_tensor(init) else torch.full((T.shape[1],), float(init), dtype=F64, device=T.device)
    ref = T.sum(0) + i0
    bound = (T.shape[0] + 64) * U32 * T.abs().sum(0) + adds * U32 * i0.abs()
    if term_err is not None:
        bound = bound + term_err.sum(0)
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------- cross-entropy
def smooth_target(labels_a, labels_b, lam, on, off, V):
    """The label form's target rows and row sum as SmoothRow evaluates them in fp32: (t [R, V] fp64, tsum [R] fp64, valid [R] bool)."""
    dev = labels_a.device
    R = labels_a.shape[0]
    a = labels_a
    b = labels_b if labels_b is not None else labels_a
    valid = (a >= 0) & (a < V) & (b >= 0) & (b < V)
    on32, off32 = torch.tensor(on, dtype=F32, device=dev), torch.tensor(off, dtype=F32, device=dev)
    lam32 = lam.float() if lam is not None else torch.ones(R, dtype=F32, device=dev)
    wa = (on32 - off32) * lam32
    wb = (on32 - off32) * (1.0 - lam32)
    cols = torch.arange(V, device=dev).unsqueeze(0)
    zero = torch.zeros((), dtype=F32, device=dev)
    t = off32 + torch.where(cols == a.unsqueeze(1), wa.unsqueeze(1), zero) + torch.where(cols == b.unsqueeze(1), wb.unsqueeze(1), zero)
    tsum = (torch.tensor(float(V), dtype=F32, device=dev) * off32).double() + (on32 - off32).double()
    return t.double(), tsum.expand(R).clone(), valid


def onehot_target(labels, V):
    valid = (labels >= 0) & (labels < V)
    cols = torch.arange(V, device=labels.device).unsqueeze(0)
    t = (cols == labels.unsqueeze(1)).double()
    return t, torch.ones(labels.shape[0], dtype=F64, device=labels.device), valid


def ce_bwd_ref(x, lse, t, tsum, scale, valid=None):
    """x [R, V] fp32 logits, lse [R] as given to the kernel, t [R, V], tsum [R], scale a [1] or [R] tensor; rows with valid False are 0 +- 0."""
    X = x.double()
    d = X - lse.double().unsqueeze(1)
    S = scale.double().reshape(-1, 1)
    tp = tsum.double().unsqueeze(1) * torch.exp(d)
    T = t.double()
    ref = (tp - T) * S
    b32 = S.abs() * U32 * (tp * (d.abs() + 4) + 2 * (tp - T).abs()) + FLUSH
    if valid is not None:
        v = valid.unsqueeze(1)
        ref, b32 = torch.where(v, ref, torch.zeros_like(ref)), torch.where(v, b32, torch.zeros_like(b32))
    return ref, b32


def ce_fwd_ref(x, t, tsum, valid=None):
    """(lse, b_lse, loss, b_loss) in fp64: loss = lse tsum - sum t x (0 +- 0 where valid is False)."""
    X = x.double()
    V = X.shape[1]
    lse = torch.logsumexp(X, 1)
    b_lse = U32 * (lse.abs() + V + 90)
    ts = tsum.double()
    tx = t.double() * X
    loss = lse * ts - tx.sum(1)
    b_loss = b_lse * ts + U32 * (V + 8) * tx.abs().sum(1)
    if valid is not None:
        loss, b_loss = torch.where(valid, loss, torch.zeros_like(loss)), torch.where(valid, b_loss, torch.zeros_like(b_loss))
    return lse, b_lse, loss, b_loss


# ------------------------------------------------------------------------------------------- inputs (shared by the host and GPU tests)
FAMILIES = ("randn2", "mean100", "spread1e-4", "spread1e4", "const", "single")


def family_rows(rows, D, seed):
    """(x fp32 [rows, D], spread [rows, 1]): row r belongs to family r % 6 -- randn * 2; mean 100, spread 1; spread 1e-4; spread 1e4; one
    constant row (var = 0); zero except one element.  spread is the size a branch output added to the row should have (0 for the last two,
    which must stay what they are)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((rows, D), generator=g)
    spread = torch.ones((rows, 1))
    for r in range(rows):
        f = r % len(FAMILIES)
        if f == 0:
            x[r] *= 2.0
            spread[r] = 2.0
        elif f == 1:
            x[r] += 100.0
        elif f == 2:
            x[r] *= 1e-4
            spread[r] = 1e-4
        elif f == 3:
            x[r] *= 1e4
            spread[r] = 1e4
        elif f == 4:
            x[r] = 0.3 + 0.1 * (r % 7)
            spread[r] = 0.0
        else:
            x[r] = 0.0
            x[r, (r * 37) % D] = 3.0
            spread[r] = 0.0
    return x, spread


def randn(shape, scale, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def ce_logits(R, V, seed):
    """fp32 [R, V]: randn * 2; row 0 scaled by 30, row 1 (when there is one) with its largest logit 100 above the rest."""
    x = randn((R, V), 2.0, seed)
    x[0] *= 30.0
    if R > 1:
        x[1, (7 * V) // 11] = float(x[1].max()) + 100.0
    return x


def plant_columns(V, label):
    """where the planted maximum goes, in turn: column 0, V - 1, V & ~3, (V & ~3) - 1 and the label (those that exist)"""
    cols = [0, V - 1, V & ~3, (V & ~3) - 1, label]
    out = []
    for c in cols:
        if 0 <= c < V and c not in out:
            out.append(c)
    return out


# -------------------------------------------------------------------------------------------------- cases (host and GPU tests alike)
BF16 = torch.bfloat16
LN_NARROW, LN_WIDE = (256, 512, 768, 1024, 1536), (2048, 3072, 8192)
LN_MODES = ("plain32", "plain16", "post16", "post32", "ls")
ROWS_BIG, ROWS_GRID = 261, 8200      # 261: 66 forward blocks, 33 backward blocks, a last block with one busy wave; 8200: past both grid caps
EPS = 1e-5


def small_rows(D, mode):
    """the second row count of a (width, mode): 1, 2, 3 or 5 -- fewer rows than a block has waves, or one block and one extra row"""
    widths = LN_NARROW + LN_WIDE
    return (1, 2, 3, 5)[(widths.index(D) + LN_MODES.index(mode)) % 4]


def ln_case(D, mode, rows, seed=0):
    """CPU tensors of one LayerNorm case.  Every mode gets rows of all six families (family_rows).  LS: rows_per_sample 50 with one zero in
    row_scale at rows = 261, 1 (zero in the last entry when rows > 1) at the small row counts, row_scale None at rows = 8200."""
    x, spread = family_rows(rows, D, 1000 + seed)
    c = {"D": D, "mode": mode, "rows": rows, "w": 1.0 + randn((D,), 0.3, 1 + seed), "b": randn((D,), 0.2, 2 + seed),
         "dy1": randn((rows, D), 1.0, 3 + seed).to(BF16), "dy2": randn((rows, D), 0.5, 4 + seed).to(BF16), "dy32": randn((rows, D), 0.5, 5 + seed),
         "dx0": randn((rows, D), 1.0, 6 + seed), "rps": 1, "row_scale": None}
    hpart = randn((rows, D), 0.5, 7 + seed) * spread
    if mode == "plain32":
        c["x"] = x
    elif mode == "plain16":
        c["x"] = x.to(BF16)
    elif mode in ("post16", "post32"):
        c["h"], c["res"] = hpart.to(BF16), (x.to(BF16) if mode == "post16" else x)
    else:
        c["x"], c["ls_gamma"] = x, 0.1 + randn((D,), 0.03, 8 + seed)
        c["h"] = (hpart / 0.1).to(BF16)
        if rows == ROWS_BIG:
            c["rps"] = 50
            c["row_scale"] = 1.0 + randn(((rows + 49) // 50,), 0.2, 9 + seed)
            c["row_scale"][2] = 0.0
        elif rows != ROWS_GRID:
            c["row_scale"] = 1.0 + randn((rows,), 0.2, 9 + seed)
            if rows > 1:
                c["row_scale"][-1] = 0.0
    return c


def ln_row(c, keep=None, drop_scale=1.0):
    """(row fp64, x_err or None) the forward of case c normalises"""
    if c["mode"].startswith("plain"):
        return c["x"].double(), None
    if c["mode"].startswith("post"):
        return post_row(c["h"], c["res"], keep, drop_scale)
    return ls_row(c["x"], c["h"], c["ls_gamma"], c["row_scale"], c["rps"])


def ln_row_f32(c):
    """the same row formed in fp32, operation by operation as the kernel forms it (no dropout)"""
    if c["mode"].startswith("plain"):
        return c["x"].float()
    if c["mode"].startswith("post"):
        return c["h"].float() + c["res"].float()
    s = row_scale_of(c["row_scale"], c["rows"], c["rps"], c["x"].device).float()
    return c["x"] + s * c["ls_gamma"] * c["h"].float()


def ln_stored(c):
    """what the backward reads as x: the row as the forward stored it (bf16 z for post16, fp32 otherwise; PLAIN: the input itself)"""
    if c["mode"].startswith("plain"):
        return c["x"]
    v = ln_row_f32(c)
    return v.to(BF16) if c["mode"] == "post16" else v


def ln_stats(xs, eps=EPS):
    """fp32 (mean, rstd) of the stored rows: the statistics handed to the backward"""
    X = xs.double()
    mu = X.mean(1)
    return mu.float(), (((X - mu.unsqueeze(1)) ** 2).mean(1) + eps).rsqrt().float()


CE_SHAPES = [(5, 50265, 50304), (9, 1001, 1008), (9, 1003, 1004), (7, 8, 8), (7, 5, 8), (4, 3, 3), (3, 4096, 4096)]
CE_FORMS = ("onehot", "label", "dense")
CE_ON, CE_OFF_MASS = 0.9, 0.1       # label form: off = 0.1 / V, so tsum = 1 - 0.1 / V < 1


def ce_case(R, V, seed=0):
    """CPU tensors of one cross-entropy case: logits (ce_logits), labels with the last row ignored, a second label and a per-row lam, a dense
    fp32 target with row sums 0.9, a scalar scale 1 / valid rows and per-row scales in (-1, 1)."""
    g = torch.Generator(device="cpu").manual_seed(50 + seed)
    labels = torch.randint(0, V, (R,), generator=g)
    labels_b = torch.randint(0, V, (R,), generator=g)
    labels[-1] = -100
    if R > 2:
        labels_b[2] = labels[2]          # both labels on one column
    lam = torch.rand((R,), generator=g)
    lam[0] = 1.0                          # the second label carries no weight
    t = torch.rand((R, V), generator=g)
    t = (t * (0.9 / t.sum(1, keepdim=True))).float()
    return {"x": ce_logits(R, V, 60 + seed), "labels": labels, "labels_b": labels_b, "lam": lam, "t": t,
            "scale1": torch.tensor([1.0 / (R - 1)]), "scaleR": torch.rand((R,), generator=g) * 2 - 1, "off": CE_OFF_MASS / V}


def ce_target(c, form, V):
    """(t, tsum, valid) of a form; the dense form's tsum is the fp32 sum a forward would hand over (here: the fp64 sum rounded)"""
    if form == "onehot":
        return onehot_target(c["labels"], V)
    if form == "label":
        return smooth_target(c["labels"], c["labels_b"], c["lam"], CE_ON, c["off"], V)
    return c["t"].double(), c["t"].double().sum(1).float().double(), None
