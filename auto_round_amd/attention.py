"""Optional attention plumbing for Hugging Face blocks on MI355X.

On ROCm 7.2 / torch 2.10 the AOTriton "efficient" SDPA kernels run the causal bf16 forward+backward of an 8x32x2048x128
problem in 2.7 ms, the "flash" ones in 5.0 ms (tools/sdpa_probe*.py).  The efficient kernels do not accept
`enable_gqa=True`, which is what transformers' stock "sdpa" path passes for grouped-query models, so torch silently
falls back to the flash kernels.  `register_mi355x_sdpa()` registers an attention function with transformers'
AttentionInterface that repeats K/V heads explicitly and calls SDPA under an efficient-first priority; select it with
`config._attn_implementation = "mi355x_sdpa"`.  Pure host-side plumbing: no arithmetic of the tuning path changes.
"""
from __future__ import annotations

import contextlib
import warnings

import torch
import torch.nn.functional as F

NAME = "mi355x_sdpa"

# (shape / stride / dtype signature of an SDPA call) -> True: the training-mode forward returned the inference-mode forward's bits
_TRAINING_FORWARD_PROVEN: dict = {}


def _sdpa_signature(query, key, value, kw):
    m = kw.get("attn_mask")
    return (tuple(query.shape), tuple(query.stride()), str(query.dtype), tuple(key.shape), tuple(value.shape),
            None if m is None else (tuple(m.shape), tuple(m.stride()), str(m.dtype)), bool(kw.get("is_causal", False)),
            kw.get("scale"), bool(kw.get("enable_gqa", False)))


# (signature) -> True: the restated forward (csrc/ar_attn_exact.hip) returned the library's bits for this kind of call
_EXACT_FORWARD_PROVEN: dict = {}
nograd_state = {"exact_calls": 0, "library_calls": 0}


def _exact_nograd_forward(query, key, value, kw):
    """The no-grad SDPA call on ar_attn_fwd_exact when it is one that kernel restates (additive mask with the calibration flow's structure,
    head size 64 / 128, S % 128 == 0): [B, H, S, D] like the library's result, or None."""
    from . import ops

    m = kw.get("attn_mask")
    if m is None or kw.get("is_causal") or kw.get("enable_gqa") or query.dim() != 4:
        return None
    B, H, S, D = query.shape
    if not (query.dtype == torch.bfloat16 and key.dtype == query.dtype and value.dtype == query.dtype and D in (64, 128) and S % 128 == 0
            and 128 <= S <= 4096 and key.shape[2] == S and value.shape == key.shape and H % key.shape[1] == 0
            and all(t.stride(3) == 1 and not any(x % 8 for x in t.stride()[:3]) and t.data_ptr() % 16 == 0 for t in (query, key, value))):
        return None
    st = ops.mask_structure(m, S)
    if st is None:
        return None
    scale = kw.get("scale")
    got = ops.attn_fwd_exact(query, key, value, st, float(scale) if scale is not None else D ** -0.5,
                             key_block=ops.attn_key_block_guess(int(D), int(S)))
    return None if got is None else got[0].transpose(1, 2)


@contextlib.contextmanager
def reproducible_sdpa_forward(enabled: bool = True, exact: bool = True):
    """Every NO-GRAD `F.scaled_dot_product_attention` call inside the context runs the library's TRAINING-mode forward (the one that
    also writes the log-sum-exp rows) instead of its inference-mode forward.

    Why (round 6, tools/gpu/r06_sdpa_flake.py, profiles/r06_sdpa_flake.json): on torch 2.10 / ROCm 7.2 / MI355X the library's
    inference-mode attention forward is NOT reproducible at OPT-125M's shape -- q / k / v [8, 12, 2048, 64] bf16 with an [8, 1, S, S]
    additive mask: 0.1-1.2 % of the calls (more when torch's deterministic-mode NaN fill or a copy precedes the call) return 16 or 32
    values that are off by 0.02-0.04, another 16 each time -- while the training-mode forward of the very same call returned the same
    bits on every one of 5 400 calls, and those bits are the inference forward's majority result.  The reference computes a block's
    TARGETS (and its quantised-output forward) under `torch.no_grad()`, i.e. through the flaky form: with 16 such calls per OPT-125M
    block about one run in seven tunes against corrupted targets (BENCH_r05's `opt125m ... targets_identical: false`).  This package's
    own no-grad forwards take the reproducible form; the values are the ones the reference gets whenever the library does not slip.

    Nothing is assumed about other shapes: the first call of every distinct signature runs BOTH forms and compares them bit for bit
    (once more if they differ: the inference form may just have slipped); a signature whose two forms differ keeps the inference form,
    with a warning.

    `exact` (end of round 6): where the restated forward kernel (csrc/ar_attn_exact.hip: the library's bits, no cross-workgroup state,
    so no race) takes the call, and its result equalled the library's on the first call of the signature, later calls run on it.  The
    training-mode forward is rarely wrong too at head size 128 -- 1 of 16 Llama-3-8B full-recipe runs computed other TARGETS
    (tools/gpu/r06_parity_repeat.py) -- and a block's targets are what the whole tuning run is measured against."""
    if not enabled:
        yield
        return
    real = F.scaled_dot_product_attention
    if getattr(real, "_ar_reproducible", False):        # nested use
        yield
        return

    def training_forward(query, key, value, a, kw):
        with torch.enable_grad():
            return real(query.detach().requires_grad_(True), key.detach(), value.detach(), *a, **kw).detach()

    def sdpa(query, key, value, *a, **kw):
        if (torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad)) or not query.is_cuda \
                or kw.get("dropout_p", 0.0) or len(a) > 0:
            return real(query, key, value, *a, **kw)
        sig = _sdpa_signature(query, key, value, kw)
        if exact:
            xok = _EXACT_FORWARD_PROVEN.get(sig)
            if xok is not False:
                o_x = _exact_nograd_forward(query, key, value, kw)
                if o_x is None:
                    if xok is None:
                        _EXACT_FORWARD_PROVEN[sig] = False
                elif xok:
                    nograd_state["exact_calls"] += 1
                    return o_x.contiguous()
                else:       # first call of the signature: the restated kernel against the library (which may slip: up to three comparisons)
                    same = False
                    for _ in range(3):
                        o_l = training_forward(query, key, value, a, kw)
                        if o_l.shape == o_x.shape and torch.equal(o_l.contiguous().view(torch.int16), o_x.contiguous().view(torch.int16)):
                            same = True
                            break
                    _EXACT_FORWARD_PROVEN[sig] = same
                    if same:
                        nograd_state["exact_calls"] += 1
                        return o_x.contiguous()
        nograd_state["library_calls"] += 1
        ok = _TRAINING_FORWARD_PROVEN.get(sig)
        if ok is None:
            same = False
            o_t = training_forward(query, key, value, a, kw)
            for _ in range(3):
                o_i = real(query, key, value, *a, **kw)
                it = {2: torch.int16, 4: torch.int32}.get(o_i.element_size())
                if it is not None and o_i.shape == o_t.shape and torch.equal(o_i.contiguous().view(it), o_t.contiguous().view(it)):
                    same = True
                    break
            ok = _TRAINING_FORWARD_PROVEN[sig] = same
            if not same:
                warnings.warn(f"reproducible_sdpa_forward: the library's training-mode attention forward differs from its inference-mode forward "
                              f"for {sig[:1]} ...; no-grad calls of this signature keep the inference form")
            return o_t if same else o_i
        return training_forward(query, key, value, a, kw) if ok else real(query, key, value, *a, **kw)

    sdpa._ar_reproducible = True
    F.scaled_dot_product_attention = sdpa
    try:
        yield
    finally:
        F.scaled_dot_product_attention = real


@contextlib.contextmanager
def guarded_sdpa(mode: str):
    """EXPERIMENT / mitigation (round 6): small device-side operations around every `F.scaled_dot_product_attention` call.  mode is a
    comma list of: "before" (a one-element kernel on the query before the call), "after" (one on the output after it), "touch" (a
    full read of the output after the call: `out.sum()` into a scratch scalar).  Same values in and out; only the launch sequence
    around the library kernel changes (tools/gpu/r06_sdpa_guard_ab.py measures what that does to run-to-run reproducibility)."""
    modes = {m.strip() for m in (mode or "").split(",") if m.strip()}
    if not modes:
        yield
        return
    real = F.scaled_dot_product_attention
    scratch = {}

    def sdpa(query, key, value, *a, **kw):
        if query.is_cuda:
            s = scratch.get(query.device)
            if s is None:
                s = scratch[query.device] = torch.zeros(4, dtype=torch.float32, device=query.device)
            if "before" in modes:
                s[0:1].add_(1.0)
            if "flush_before" in modes or "flush_after" in modes:
                big = scratch.get("big")
                if big is None:
                    big = scratch["big"] = torch.zeros(1 << 25, dtype=torch.float32, device=query.device)      # 128 MB read + written
            if "flush_before" in modes:
                big.add_(1.0)
            if "touch_inputs" in modes:          # read q / k / v / mask right before the call (pull them towards the caches)
                with torch.no_grad():
                    m = kw.get("attn_mask")
                    acc = query.detach().float().sum() + key.detach().float().sum() + value.detach().float().sum()
                    if m is not None:
                        acc = acc + m.float().sum()
                    s[3:4].copy_(acc.reshape(1))
            if "sync_before" in modes:
                torch.cuda.synchronize(query.device)
        out = real(query, key, value, *a, **kw)
        if query.is_cuda:
            if "sync_after" in modes:
                torch.cuda.synchronize(query.device)
            if "flush_after" in modes:
                big.add_(1.0)
            if "after" in modes:
                s[1:2].add_(1.0)
            if "touch" in modes:
                with torch.no_grad():
                    s[2:3].copy_(out.detach().float().sum().reshape(1))
        return out

    F.scaled_dot_product_attention = sdpa
    try:
        yield
    finally:
        F.scaled_dot_product_attention = real


@contextlib.contextmanager
def verified_sdpa_forward(flag: torch.Tensor):
    """Every GRAD-MODE `F.scaled_dot_product_attention` call inside the context is issued TWICE (the second one detached, same
    training-mode kernel) and `flag` (a one-element device tensor) is set when the two results differ in any bit -- no host
    synchronisation.  The library's attention forward slips about once in 4000 calls at OPT-125M's shape even in its training-mode
    form (profiles/r06_opt_loop_flake2.json: the one op of a tuning iteration that is not reproducible); a tuning run whose flag is
    set at the end has -- or may have -- taken a corrupted step and is repeated by the caller (`SignRoundConfig.
    verify_attention_forward`), which makes the tuned block a deterministic function of its inputs on a library that is not."""
    real = F.scaled_dot_product_attention

    def sdpa(query, key, value, *a, **kw):
        out = real(query, key, value, *a, **kw)
        if torch.is_grad_enabled() and out.requires_grad and query.is_cuda and not kw.get("dropout_p", 0.0):
            with torch.enable_grad():
                again = real(query.detach().requires_grad_(True), key.detach(), value.detach(), *a, **kw).detach()
            it = {2: torch.int16, 4: torch.int32}.get(out.element_size())
            if it is not None:
                flag.logical_or_((out.detach().view(it) != again.view(it)).any())
        return out

    F.scaled_dot_product_attention = sdpa
    try:
        yield
    finally:
        F.scaled_dot_product_attention = real


def efficient_backward_ok(seq: int) -> bool:
    """torch 2.10 + ROCm 7.2: the backward of the "efficient" SDPA kernels (aiter fmha_bwd behind AOTriton) returns wrong
    gradients (relative error ~1, NaNs) for token-major [B, S, H, D] operands when S % 256 == 128 and S > 128 (384, 640, 896, ...);
    contiguous [B, H, S, D] operands and every other length checked are right, and so are the "flash" and "math" backends
    (measured against fp32 autograd: tools/sdpa_backward_check.py, profiles/archive/r02_sdpa_backward_check.json).  Callers route those
    lengths to the flash kernels."""
    return seq <= 128 or seq % 256 != 128


def backend_order(prefer: str, seq=None):
    from torch.nn.attention import SDPBackend

    if prefer == "math":
        return [SDPBackend.MATH]
    if prefer == "flash" or (seq is not None and not efficient_backward_ok(int(seq))):
        return [SDPBackend.FLASH_ATTENTION, SDPBackend.MATH] if prefer != "flash" else [SDPBackend.FLASH_ATTENTION,
                                                                                       SDPBackend.EFFICIENT_ATTENTION, SDPBackend.MATH]
    return [SDPBackend.EFFICIENT_ATTENTION, SDPBackend.FLASH_ATTENTION, SDPBackend.MATH]


def _repeat_kv(x: torch.Tensor, n_rep: int) -> torch.Tensor:
    if n_rep == 1:
        return x
    b, h, s, d = x.shape
    return x[:, :, None, :, :].expand(b, h, n_rep, s, d).reshape(b, h * n_rep, s, d)


def mi355x_sdpa_attention(module, query, key, value, attention_mask=None, dropout=0.0, scaling=None, is_causal=None,
                          **kwargs):
    from torch.nn.attention import SDPBackend, sdpa_kernel

    n_rep = getattr(module, "num_key_value_groups", 1)
    key, value = _repeat_kv(key, n_rep), _repeat_kv(value, n_rep)
    if attention_mask is not None and attention_mask.ndim == 4:
        attention_mask = attention_mask[:, :, :, : key.shape[-2]]
    if is_causal is None:
        is_causal = query.shape[2] > 1 and attention_mask is None and getattr(module, "is_causal", True)
    order = backend_order("efficient", query.shape[2])
    with sdpa_kernel(order, set_priority=True):
        out = F.scaled_dot_product_attention(query, key, value, attn_mask=attention_mask, dropout_p=dropout,
                                             scale=scaling, is_causal=bool(is_causal))
    return out.transpose(1, 2).contiguous(), None


def register_mi355x_sdpa() -> str:
    from transformers import AttentionInterface

    AttentionInterface.register(NAME, mi355x_sdpa_attention)
    return NAME


# ---- the module path's attention on the first-party kernels with the library's bits (round 6) ---------------------------------------
EXACT_NAME = "mi355x_exact_sdpa"
# verify: torch's own attention runs beside every call and the outputs / gradients are compared (the quantizer's proof);
# materialise: the caller hands the shared one-row mask over un-materialised -- a fallback call expands it as the module path would
exact_state = {"verify": False, "diffs": {}, "calls": 0, "fallbacks": 0, "materialise": False, "key_block": 0}


class _ExactAttnFn(torch.autograd.Function):
    """q [B, H, S, D], k / v [B, H / kv_rep, S, D] (un-repeated: transformers' repeat_kv only copies) -> out [B, S, H, D];
    csrc/ar_attn_exact.hip forward and backward.  `ref` (proof runs only): torch's own attention on detached leaves."""

    @staticmethod
    def forward(ctx, q, k, v, st, scale, ref):
        from . import ops
        from .exact_proof import count_diff

        kb = int(exact_state.get("key_block") or 0) or ops.attn_key_block_guess(int(q.shape[-1]), int(q.shape[2]))
        got = ops.attn_fwd_exact(q, k, v, st, float(scale), key_block=kb)
        if got is None:
            raise RuntimeError("ar_attn_fwd_exact refused a call its caller checked")
        o, lse = got
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.st, ctx.scale, ctx.ref = st, float(scale), ref
        if ref is not None:
            d = exact_state["diffs"]
            d["out"] = d.get("out", 0) + count_diff(o, ref[3].detach())
        return o

    @staticmethod
    def backward(ctx, do):
        from .exact_proof import count_diff, exact_attention_backward      # (lazy: exact_proof does not import this module)

        q, k, v, o, lse = ctx.saved_tensors
        if do.stride(-1) != 1 or any(s % 8 for s in do.stride()[:3]):
            do = do.contiguous()
        gq, gk, gv = exact_attention_backward((q, k, v, o, lse, ctx.st), do, ctx.scale)
        if ctx.ref is not None:
            ql, kl, vl, ro = ctx.ref
            d = exact_state["diffs"]
            for name, mine, want in zip(("dq", "dk", "dv"), (gq, gk, gv), torch.autograd.grad(ro, (ql, kl, vl), do)):
                d[name] = d.get(name, 0) + count_diff(mine, want)
        return gq, gk, gv, None, None, None


def exact_sdpa_attention(module, query, key, value, attention_mask=None, dropout=0.0, scaling=None, is_causal=None, **kwargs):
    """transformers attention function (AttentionInterface) for the MODULE PATH: the call `sdpa_attention_forward` would hand to
    torch's SDPA runs on ar_attn_fwd_exact / ar_attn_bwd_exact when it is one those kernels restate (the calibration flow's structured
    additive mask, head size 64 / 128, S % 128 == 0, no dropout) -- the library's bits, proven per block by the quantizer before this
    function is installed -- and on `sdpa_attention_forward` itself for anything else."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    from . import ops

    B, H, S, D = query.shape
    st = None
    if (not dropout and attention_mask is not None and query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == query.dtype
            and value.dtype == query.dtype and D in (64, 128) and S % 128 == 0 and S <= 4096 and key.shape[2] == S
            and kwargs.get("position_bias") is None and not kwargs.get("output_attentions", False)
            and all(t.stride(3) == 1 and not any(x % 8 for x in t.stride()[:3]) and t.data_ptr() % 16 == 0 for t in (query, key, value))):
        st = ops.mask_structure(attention_mask, S)
    if st is None:
        exact_state["fallbacks"] += 1
        if exact_state["materialise"] and attention_mask is not None and attention_mask.shape[0] == 1 and B > 1:
            attention_mask = attention_mask.expand(B, *attention_mask.shape[1:]).contiguous()
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, is_causal=is_causal, **kwargs)
    exact_state["calls"] += 1
    scale = float(scaling) if scaling is not None else D ** -0.5
    ref = None
    if exact_state["verify"]:
        with torch.enable_grad():
            ql, kl, vl = (t.detach().requires_grad_(True) for t in (query, key, value))
            mask = attention_mask
            if exact_state["materialise"] and mask.shape[0] == 1 and B > 1:
                mask = mask.expand(B, *mask.shape[1:]).contiguous()
            ro, _ = sdpa_attention_forward(module, ql, kl, vl, mask, dropout=0.0, scaling=scaling, is_causal=is_causal, **kwargs)
        ref = (ql, kl, vl, ro)
    return _ExactAttnFn.apply(query, key, value, st, scale, ref), None


def register_exact_sdpa() -> str:
    from transformers import AttentionInterface

    AttentionInterface.register(EXACT_NAME, exact_sdpa_attention)
    return EXACT_NAME
