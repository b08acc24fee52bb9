"""Cases shared by the host check (tests/test_attn_exact_cases_host.py) and the GPU edge tests (tests/test_gpu_attn_exact_edges.py)
of the restated attention (csrc/ar_attn_exact.hip): the case tables, the dense form of the structured mask, the operand layouts the
callers pass, a plain fp64 attention (the arbiter when the kernel and torch differ) and the kernels' own classification of a
(query, key) pair's tile.  Imported, not collected."""
import collections

import torch

# head size -> (softmax scale, operand std): tests/test_gpu_attn_exact.py's settings
SETTINGS = {128: (128 ** -0.5, 1.0), 64: (1.0, 0.35)}
DOUT_STD = 0.02

BIAS_PAIRS = [(1.0, 0.0), (0.0, 1.0), (0.5, -2.0), (3.0, -2.5), (0.8125, -0.0078125), (0.0, -8192.0), (-3.0, 0.0)]

# (B, H, hk, S, D): the smallest shapes that select each kernel form
GRID_SHAPES = {
    "d128-s384-ungrouped": (2, 2, 2, 384, 128),      # forward 4 waves, key block 32; query side 4 waves; one-shot key side
    "d128-s512-rep2": (2, 4, 2, 512, 128),           # forward and query side 8 waves; grouped key side, groups of up to 4
    "d128-s384-rep8": (1, 8, 1, 384, 128),           # grouped key side, groups of 8
    "d128-s640-keyblock64": (1, 2, 2, 640, 128),     # forward key block 64, 4 waves
    "d128-s768-keyblock64": (1, 2, 2, 768, 128),     # forward key block 64, 8 waves
    "d64-s256-rep2": (1, 4, 2, 256, 64),             # head size 64: per-head key side and torch's sum over the group
    "d64-s640-keyblock32": (1, 2, 2, 640, 64),       # head size 64, key block 32
}
# refused by both launchers (the caller keeps torch's SDPA): head size 64 at S = 128 -- the forward equals torch there, the backward does
# not (1 to 9 of 32768 dq / dk / dv values differ at every valid length: the library runs another configuration), so the pair is refused
REFUSED_SHAPES = {"d64-s128": (2, 2, 2, 128, 64)}
BIAS_SHAPES = {"d128-s512-rep2": (2, 4, 2, 512, 128), "d128-s384-rep8": (1, 8, 1, 384, 128), "d64-s256-rep2": (1, 4, 2, 256, 64)}
LAYOUT_SHAPES = [(2, 8, 2, 384, 128), (2, 8, 1, 384, 128), (2, 4, 4, 256, 64)]
LAYOUTS = ["head_major", "qkv_slices", "dout_slice", "outs_slices"]
# name -> (shape, head-scaled dout): kv_rep 3 (the grouped kernel takes it), 6 (refused: per-head kernel and torch's sum), 1 with grouped=True
GROUP_CASES = {
    "rep3": ((1, 6, 2, 384, 128), False),
    "rep6": ((1, 12, 2, 384, 128), False),
    "rep1-grouped": ((1, 2, 2, 384, 128), False),
    "rep3-head-scaled": ((1, 6, 2, 384, 128), True),
}
VALUE_SHAPES = [(1, 4, 2, 384, 128), (1, 4, 4, 256, 64)]
# "sink" scales by 16 (scores in the thousands: every row's whole mass on one key), "sink_mild" by 4 (the largest scores at several tens)
VALUE_FAMILIES = ["sink", "sink_mild", "saturation", "degenerate"]

Case = collections.namedtuple("Case", "shape valid bias layout family head_scaled")


def valid_grid(S):
    """valid lengths on, one under and one over the 32- and 64-row boundaries the kernels classify tiles by, at both ends of the sequence"""
    cand = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 192, 193, S - 65, S - 64, S - 63, S - 33, S - 32, S - 1, S]
    return sorted({v for v in cand if 1 <= v <= S})


def _case(shape, valid, bias=(1.0, 0.0), layout="token", family="randn", head_scaled=False):
    return Case(tuple(shape), int(valid), tuple(bias), layout, family, bool(head_scaled))


def grid_cases(name):
    shape = GRID_SHAPES[name]
    return [_case(shape, v) for v in valid_grid(shape[3])]


def refused_cases(name):
    shape = REFUSED_SHAPES[name]
    return [_case(shape, v) for v in valid_grid(shape[3])]


def bias_cases(name):
    shape = BIAS_SHAPES[name]
    S = shape[3]
    return [_case(shape, v, bias) for bias in BIAS_PAIRS for v in (1, S // 2 + 1, S)]


def layout_cases(layout):
    return [_case(shape, shape[3] - 33, layout=layout) for shape in LAYOUT_SHAPES]


def group_cases(name):
    shape, head_scaled = GROUP_CASES[name]
    return [_case(shape, v, head_scaled=head_scaled) for v in (shape[3] - 1, 193)]


def value_cases(family):
    return [_case(shape, v, family=family) for shape in VALUE_SHAPES for v in (shape[3] - 1, 129)]


def all_tables():
    """{test id: [Case]} -- every case the GPU tests run; both test files take their cases (and their count) from here"""
    out = {}
    for n in GRID_SHAPES:
        out["grid/" + n] = grid_cases(n)
    for n in REFUSED_SHAPES:
        out["refused/" + n] = refused_cases(n)
    for n in BIAS_SHAPES:
        out["bias/" + n] = bias_cases(n)
    for n in LAYOUTS:
        out["layout/" + n] = layout_cases(n)
    for n in GROUP_CASES:
        out["group/" + n] = group_cases(n)
    for n in VALUE_FAMILIES:
        out["values/" + n] = value_cases(n)
    return out


def dense_mask(B, S, valid, b_in, b_out, device="cpu"):
    """the structured additive mask as the calibration flow hands it over: bf16 [B, 1, S, S] contiguous, `b_in` where
    `key <= query and key < valid`, `b_out` elsewhere"""
    idx = torch.arange(S, device=device)
    keep = (idx[None, :] <= idx[:, None]) & (idx[None, :] < valid)
    m = torch.where(keep, torch.tensor(float(b_in), device=device), torch.tensor(float(b_out), device=device)).to(torch.bfloat16)
    return m[None, None].expand(B, 1, S, S).contiguous()


def fp64_attention(q, k, v, mask, scale, dout):
    """plain fp64 attention on the operands' device: s = (q k^T) * scale + mask, lse = logsumexp(s), o = softmax(s) v, gradients by
    autograd.  q [B, H, S, D], k / v [B, hk, S, D] (repeat_kv by expand), mask [B, 1, S, S], dout [B, S, H, D].
    -> (o [B, S, H, D], lse [B, H, S], dq [B, H, S, D], dk, dv [B, hk, S, D]), all fp64.  Asserts nothing: the arbiter and the diagnostic."""
    B, H, S, D = q.shape
    hk = k.shape[1]
    rep = H // hk
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    ke = kd[:, :, None].expand(B, hk, rep, S, D).reshape(B, H, S, D)
    ve = vd[:, :, None].expand(B, hk, rep, S, D).reshape(B, H, S, D)
    s = (qd @ ke.transpose(-1, -2)) * float(scale) + mask.double()
    lse = torch.logsumexp(s, dim=-1)
    o = (torch.softmax(s, dim=-1) @ ve).transpose(1, 2)
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), dout.double())
    return o.detach(), lse.detach(), dq, dk, dv


def tile_class(query, key, valid):
    """how the kernels classify the tile a (query, key) pair falls into: -> (forward and backward MODE 0 (query side), backward MODE 1
    (key side)), each "plain" (every pair of the tile inside the kept region), "all_out" (every pair outside) or "mixed" (the per-element
    choice) -- the conditions of csrc/ar_attn_exact.hip written out.
    Forward / MODE 0: a wave owns 32 query rows from w0 and meets tiles of 64 keys from k0.  MODE 1: a wave owns 32 key rows from o and
    meets tiles of 64 queries from t0."""
    w0, k0 = query // 32 * 32, key // 64 * 64
    if k0 + 63 <= w0 and k0 + 64 <= valid:
        qside = "plain"
    elif k0 > w0 + 31 or k0 >= valid:
        qside = "all_out"
    else:
        qside = "mixed"
    o, t0 = key // 32 * 32, query // 64 * 64
    if t0 >= o + 31 and o + 31 < valid:
        kside = "plain"
    elif o > t0 + 63 or o >= valid:
        kside = "all_out"
    else:
        kside = "mixed"
    return qside, kside


def row_classes(row, S, valid, key_side):
    """the classes of every tile a wave meets along one row, in tile order, one letter each (P plain, O all_out, M mixed): for a query
    row the 64-key tiles of the forward / MODE 0, for a key row (key_side) the 64-query tiles of MODE 1"""
    letter = {"plain": "P", "all_out": "O", "mixed": "M"}
    if key_side:
        return "".join(letter[tile_class(t0, row, valid)[1]] for t0 in range(0, S, 64))
    return "".join(letter[tile_class(row, k0, valid)[0]] for k0 in range(0, S, 64))


def operands(case, device="cpu", seed=None):
    """the operands of a case in its layout: {"q", "k", "v"}: [B, heads, S, D] bf16 views, "dout": a [B, S, H, D] view, "outs": None or
    the (dq, dk, dv) destinations, "wide": the buffer the destinations are slices of, "gaps": its column ranges outside them,
    "max_score": the largest q k^T * scale.  The values depend on (shape, family, head_scaled) only, never on the layout or the mask."""
    B, H, hk, S, D = case.shape
    rep = H // hk
    std = SETTINGS[D][1]
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + S + H if seed is None else seed)

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    if case.family == "saturation":                # p is 0 or 1 almost everywhere, alpha underflows
        std = 4 * std
    q, k, v = randn(B, S, H, D) * std, randn(B, S, hk, D) * std, randn(B, S, hk, D)
    do = randn(B, S, H, D) * DOUT_STD
    if case.family in ("sink", "sink_mild"):       # an attention sink: key 0 and four random channels of q and k scaled up
        f = 16 if case.family == "sink" else 4
        ch = torch.randperm(D, generator=g)[:4]
        k[:, 0] *= f
        q[..., ch] *= f
        k[..., ch] *= f
    if case.family == "degenerate":                # 32 queries exactly zero across a wave boundary, the next 32 negative zero; one head without gradient
        q[:, 80:112] = 0.0
        q[:, 112:144] = -0.0
        do[:, :, H - 1] = 0.0
    if case.head_scaled:                           # query head j of a group weighs 2^(-10 j): the order of the group's sum shows in the bits
        w = torch.tensor([2.0 ** (-10 * (j % rep)) for j in range(H)])
        do = do * w[None, None, :, None]
    q, k, v, do = (t.to(torch.bfloat16).to(device) for t in (q, k, v, do))
    hd, hkd = H * D, hk * D
    res = {"outs": None, "wide": None, "gaps": []}
    if case.layout == "qkv_slices":                # three column slices of one merged buffer, from column 8
        buf = torch.zeros(B * S, hd + 2 * hkd + 16, dtype=torch.bfloat16, device=device)
        cols = [(8, hd, H), (8 + hd, hkd, hk), (8 + hd + hkd, hkd, hk)]
        views = []
        for t, (c0, n, nh) in zip((q, k, v), cols):
            buf[:, c0:c0 + n] = t.reshape(B * S, n)
            views.append(buf[:, c0:c0 + n].view(B, S, nh, D).transpose(1, 2))
        res["q"], res["k"], res["v"] = views
    elif case.layout == "head_major":              # [B, heads, S, D] contiguous: the module path's tensors
        res["q"], res["k"], res["v"] = (t.transpose(1, 2).contiguous() for t in (q, k, v))
    else:                                          # token-major [B, S, heads, D], as the direct tests pass
        res["q"], res["k"], res["v"] = (t.transpose(1, 2) for t in (q, k, v))
    if case.layout == "dout_slice":                # the output gradient as a view of a column slice of a wider 2-D buffer
        dbuf = torch.zeros(B * S, hd + 16, dtype=torch.bfloat16, device=device)
        dbuf[:, 8:8 + hd] = do.reshape(B * S, hd)
        res["dout"] = dbuf[:, 8:8 + hd].view(B, S, H, D)
    else:
        res["dout"] = do
    if case.layout == "outs_slices":               # dq / dk / dv into column slices of one wider gradient buffer
        wide = torch.full((B * S, hd + 2 * hkd + 32), 7.0, dtype=torch.bfloat16, device=device)
        c = [8, 16 + hd, 24 + hd + hkd]
        res["outs"] = (wide[:, c[0]:c[0] + hd], wide[:, c[1]:c[1] + hkd], wide[:, c[2]:c[2] + hkd])
        res["wide"] = wide
        res["gaps"] = [(0, 8), (8 + hd, 16 + hd), (16 + hd + hkd, 24 + hd + hkd), (24 + hd + 2 * hkd, 32 + hd + 2 * hkd)]
    qf = res["q"].float()
    kf = res["k"].float()[:, :, None].expand(B, hk, rep, S, D).reshape(B, H, S, D)
    res["max_score"] = float((qf @ kf.transpose(-1, -2)).max()) * SETTINGS[D][0]
    return res
