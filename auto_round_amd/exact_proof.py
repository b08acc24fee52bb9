"""`exact_rounding`: the PROOF that a block on first-party kernels carries the module path's bits, written once for every block family
(exact_block.py: Llama family; exact_opt_block.py: OPT family) and for the module path's own attention swap (quantizer.py
`_install_module_attention`).

The policy:
  * the reference is the module code itself on real minibatches: forward, the loop's own loss gradient, backward, on frozen state
    (`reference_run`);
  * a trial plan is compared with it value for value -- block output and every arena's weight gradients (`Proof.mismatches`) -- and
    joins the plan only after TWO CONSECUTIVE runs with nothing differing, the second on the last minibatch (`Proof.proven`);
  * the attention option is also held to torch's attention DIRECTLY: output, dQ, dK, dV of every call, compared inside the segment
    (`Proof.proven_attention`, `attn_direct_ok`);
  * whatever is dropped is loud: `warnings.warn` and `plan_report` (`Proof.finish`).

What a family adds is its option list and who gets which variants and how many pairs of runs: those loops stay in the family's class
and call the pieces here.  `ExactBlockMixin` carries what the two classes share outside the search: the state a proof drives
(`_attn_verify`, `_attn_diffs`, `plan_report`), the context the module path runs under, and the attention segment -- torch's SDPA in
a local autograd graph or csrc/ar_attn_exact.hip, with torch beside the kernel while a proof runs."""
from __future__ import annotations

import contextlib
import types
import warnings
from typing import Optional

import torch

from . import ops
from .fused_block import _FusedBlockFn

ATTN_DIRECT_KEYS = {"out", "dq", "dk", "dv"}


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def count_diff(a: torch.Tensor, b: torch.Tensor) -> int:
    """number of values whose bits differ (everything, when the shapes or dtypes do)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return int(max(a.numel(), b.numel()))
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return int((a.contiguous().view(it) != b.contiguous().view(it)).sum())


def reset_dw_accum(arenas):
    """the next weight-gradient GEMM of every layer overwrites (a run that was compared must not accumulate into the next)"""
    for a in arenas:
        for l in a.layers:
            l._dw_accum[0] = False


def reference_run(module_forward, arenas, xb, ob, rb):
    """One minibatch through the MODULE PATH as the tuning loop runs it: forward, the loss gradient of ops.mse_loss_fwd_bwd against the
    targets `rb`, backward into the arenas.  -> (dpred, prediction, a copy of every arena's weight gradients)"""
    reset_dw_accum(arenas)
    pred = module_forward(xb, ob)
    pred_c = pred if pred.is_contiguous() else pred.contiguous()
    dpred = torch.empty_like(pred_c)
    scratch = torch.zeros(1, dtype=torch.float32, device=xb.device)
    ops.mse_loss_fwd_bwd(pred_c, rb.to(pred_c.dtype), dpred=dpred, loss_accum=scratch, accum_scale=1.0, grad_scale=1000.0)
    pred_c.backward(dpred)
    return dpred, pred_c.detach(), [a.dWq.clone() for a in arenas]


def run_diff(y, dws, y_ref, dw_ref) -> int:
    """number of values of the block output and of every weight gradient that differ from the reference's"""
    return count_diff(y, y_ref) + sum(count_diff(a, b) for a, b in zip(dws, dw_ref))


def key_block_candidates(guess: int):
    """the attention forward's key blocks in the order a proof tries them: 0 (= the measured guess for the shape,
    ops.attn_key_block_guess), then the library's other configurations"""
    return [0] + [b for b in (64, 32, 16) if b != guess]


def attn_direct_ok(direct: dict) -> bool:
    """the direct comparison with torch's attention: every one of output, dQ, dK, dV was compared, and nothing differed"""
    return set(direct) == ATTN_DIRECT_KEYS and not any(direct.values())


def attention_forward_same(eb, same, plan, runs: int) -> bool:
    """forward-only attention trial: `runs` consecutive forwards equal to the module path's (`same`), torch's attention beside the
    kernel in each, and its output compared at all and equal"""
    eb._attn_verify, eb._attn_diffs = True, {}
    ok = all(same(plan) for _ in range(runs))
    eb._attn_verify = False
    return ok and eb._attn_diffs.get("out", -1) == 0


class Proof:
    """One exact block `eb` against the module path's recorded results on `minibatches` = [(x, others, targets), ...] ([rows, S, H]
    each, the loop's real minibatch shape: the library picks its GEMM kernels by shape).  The family's search asks `proven(plan)` /
    `proven_attention(plan)` per trial, writes what it tried into `report`, and ends with `refuse` or `finish`."""

    def __init__(self, eb, module_forward, minibatches):
        self.eb = eb
        for a in eb.arenas:
            if not a.wq_fresh:
                a.qdq_forward()
        self.mbs = [(xb, ob) + reference_run(module_forward, eb.arenas, xb, ob, rb) for xb, ob, rb in minibatches]
        self.report = dict(errors={}, tried=[], kept=[], skipped={}, dropped={}, minibatches=len(self.mbs))

    def mismatches(self, plan, mb=0) -> int:
        """number of values of the block output and of every weight gradient that differ from the module path's (-1: the form
        refused the shape)"""
        xb, ob, dpred, y_ref, dw_ref = self.mbs[mb]
        self.eb.set_plan(plan)
        try:
            y, dws = self.eb._run_once(xb, ob, dpred)
        except (RuntimeError, ValueError, NotImplementedError) as e:      # a kernel refusing the shape: not an option here
            self.report["errors"][",".join(k for k, v in plan.items() if v)] = repr(e)[:200]
            return -1
        return run_diff(y, dws, y_ref, dw_ref)

    def proven(self, plan):
        """two consecutive runs without a differing value -> (True, 0), else (False, differing values of the run that failed).
        Acceptance (round 5): the second run is on the second minibatch when there is one, so that a form that is only
        usually equal, or an intermittent first-party defect, cannot pass as "1 of 2"."""
        n = self.mismatches(plan, 0)
        if n != 0:
            return False, n
        n = self.mismatches(plan, len(self.mbs) - 1)
        return n == 0, n

    def proven_attention(self, plan, **tag):
        """`proven` with torch's attention running beside the kernels: outputs and gradients compared directly (what differed goes to
        report["attn_direct"], with the caller's `tag`), and equal block bits without all four direct comparisons at zero is a failure"""
        eb = self.eb
        eb._attn_verify, eb._attn_diffs = True, {}
        ok, n_bad = self.proven(plan)
        eb._attn_verify = False
        direct = dict(eb._attn_diffs)
        self.report.setdefault("attn_direct", []).append(dict(direct, **tag))
        if not attn_direct_ok(direct):
            ok, n_bad = False, (n_bad if n_bad else sum(direct.values()) or -1)
        return ok, n_bad

    def kept_on_second_try(self, opt, worst, warn=True):
        self.report.setdefault("kept_on_second_try", []).append(opt)
        if warn:
            warnings.warn(f"exact_rounding: option {opt} differed from the module path in its first pair of runs ({worst}) and "
                          f"matched in the second pair -- kept; the library under the comparison is not perfectly repeatable")

    def refuse(self, n_bad) -> None:
        """not even the all-torch form reproduces the module path: the caller keeps the module path"""
        reset_dw_accum(self.eb.arenas)
        self.eb.plan_report = dict(self.report, usable=False, base_mismatches=n_bad)
        warnings.warn(f"exact_rounding: even with every segment on torch's own ops {type(self.eb.block).__name__} differs from the module "
                      f"path ({n_bad} values); blocks of this kind keep the module path")
        return None

    def finish(self, plan, is_int, left_on: str, per: str):
        """install `plan` and write `plan_report`; every dropped option (with the number of differing values) is reported through
        `warnings.warn` too -- a library bump must not cost 20 % silently.  is_int(key): the plan value is a
        number, not a switch; left_on / per: the family's words for where a dropped option stays and what was counted."""
        eb, report = self.eb, self.report
        if report["dropped"]:
            warnings.warn(f"exact_rounding: {type(eb.block).__name__}: not bit-equal to the module path on this stack and left on {left_on} "
                          f"(slower): {report['dropped']} (differing values per tried {per})")
        eb.set_plan(plan)
        reset_dw_accum(eb.arenas)
        eb.plan_report = dict(report, usable=True, plan={k: (int(v) if is_int(k) else bool(v)) for k, v in plan.items()})
        return plan


# ---- the attention with the library's bits -----------------------------------------------------------------------------------------
def exact_attention_forward(q4, k4, v4, mask, scale, S, key_block=0):
    """first-party attention with the library's bits (ops.attn_fwd_exact) when the call is one it takes: the calibration flow's
    structured additive mask, head size 64 / 128, a sequence the backward kernels take too.  -> (q4, k4, v4, out [B, S, H, D], lse,
    mask_struct) or None"""
    if mask is None or S % 128 or S > 4096:
        return None
    st = ops.mask_structure(mask, S)
    if st is None:
        return None
    kb = int(key_block) or ops.attn_key_block_guess(int(q4.shape[-1]), int(S))
    got = ops.attn_fwd_exact(q4, k4, v4, st, float(scale), key_block=kb)
    if got is None:
        return None
    return (q4, k4, v4, got[0], got[1], st)


def exact_attention_backward(xa, dattn4, scale, outs=None):
    """gradients of the call `exact_attention_forward` made: -> (gq4 [B, H, S, D], gk4, gv4 [B, H / kv_rep, S, D]) -- the kv_rep query
    heads of a group summed as autograd's expand backward does (one fp32 sum per value, rounded once): inside the key-side kernel
    at head size 128 with groups of up to 4, or of 8 (ops.attn_bwd_exact grouped), by torch's sum over the per-head results otherwise.
    outs: (dq [B * S, H * D], dk, dv [B * S, (H / kv_rep) * D]) destinations the kernels write into (column slices of a merged
    gradient buffer; any of them None: a fresh buffer); ignored on the path that sums per-head results."""
    q4, k4, v4, o4, lse, st = xa
    B, H, S, D = q4.shape
    hk = k4.shape[1]
    kw = {} if outs is None else dict(dq=outs[0], dk=outs[1], dv=outs[2])
    if hk < H:
        got = ops.attn_bwd_exact(q4, k4, v4, o4, lse, dattn4, st, float(scale), grouped=True, **kw)
        if got is not None:
            return got[0].transpose(1, 2), got[1].transpose(1, 2), got[2].transpose(1, 2)
        kw = {}
    got = ops.attn_bwd_exact(q4, k4, v4, o4, lse, dattn4, st, float(scale), **kw)
    if got is None:
        raise RuntimeError("ar_attn_bwd_exact refused a call whose forward it took")
    dq, dke, dve = (t if t.dim() == 4 else t.view(B, S, H, D) for t in got)
    gq4 = dq.transpose(1, 2)
    if hk == H:
        return gq4, dke.transpose(1, 2), dve.transpose(1, 2)
    rep = H // hk
    gk4 = dke.transpose(1, 2).reshape(B, hk, rep, S, D).sum(2)
    gv4 = dve.transpose(1, 2).reshape(B, hk, rep, S, D).sum(2)
    return gq4, gk4, gv4


class ExactBlockMixin:
    """What the exact block classes share around their own arithmetic (they list it before their fused base class)."""
    capturable = False          # the attention runs in a local autograd graph: the iteration is host-driven
    exact = True
    _attn_verify = False        # a proof is running: torch's attention beside the first-party one, what differs counted in `_attn_diffs`
    _attn_diffs: dict = {}      # (class-level defaults: only a proof writes, and it installs its own dictionary first)

    def _init_exact_state(self, amp, plain=None):
        """plain: {key: nn.Linear} of an UNWRAPPED block (the no-grad form) -- the layers as the wrapped form names them"""
        if plain is not None:
            self.layers = {n: types.SimpleNamespace(weight_q=m.weight, orig_layer=m) for n, m in plain.items()}
        self.amp = bool(amp)
        self.plan = self.base_plan()
        self.plan_report: Optional[dict] = None
        self._attn_verify = False
        self._attn_diffs = {}

    def _ctx(self, S):
        """what the module path runs under: the quantizer's SDPA backend choice and (with amp) autocast"""
        st = contextlib.ExitStack()
        if self.sdpa_ctx is not None:
            st.enter_context(self.sdpa_ctx(S))
        if self.amp:      # (o: a projection every family names alike)
            st.enter_context(torch.autocast(device_type=self.layers["o"].weight_q.device.type, dtype=self.dtype))
        return st

    def _bias(self, key):
        b = self.layers[key].orig_layer.bias
        return None if b is None else b.to(self.dtype)

    @staticmethod
    def _dw_written(lyrs):
        """after a weight-gradient GEMM into the arena rows of `lyrs`: the next one accumulates, and the layer's own epilogue runs"""
        for lyr in lyrs:
            lyr._dw_accum[0] = True
            post = getattr(lyr, "_post_dw", None)
            if post is not None:
                post()

    def _run_once(self, x, others, dpred):
        reset_dw_accum(self.arenas)
        y = _FusedBlockFn.apply(x, self.arena.token, self, others)
        y.backward(dpred)
        return y.detach(), [a.dWq.clone() for a in self.arenas]

    def _forward_same(self, plan, x, others, y_ref) -> bool:
        """forward-only trial: this class's output under `plan` equal to the module path's `y_ref`, bit for bit"""
        self.set_plan(plan)
        try:
            return bits_equal(self._forward_impl(x, others, None).detach(), y_ref)
        except (RuntimeError, ValueError, NotImplementedError):
            return False

    # -- the attention segment ---------------------------------------------------------------------------------------------
    def _attention_forward(self, q4, k4, v4, mask, scale, grad):
        """q4 [B, hq, S, hd], k4 / v4 [B, hkv, S, hd] (views of token-major GEMM outputs) -> (attention output [B * S, hq * hd],
        what `_attention_backward` needs): transformers' own sdpa_attention_forward on the layouts the module hands over, in a local
        autograd graph -- or (plan["attn"]) the first-party kernels; with `_attn_verify` both, compared."""
        from transformers.integrations.sdpa_attention import sdpa_attention_forward

        P = self.plan
        B, hq, S, hd = q4.shape
        xa = exact_attention_forward(q4, k4, v4, mask, scale, S, P.get("attn_kb", 0)) if P.get("attn") else None
        al = ao = None
        if xa is None and mask is not None and getattr(self, "materialise_mask_rows", False) and mask.shape[0] == 1 and B > 1:
            mask = mask.expand(B, *mask.shape[1:]).contiguous()      # (the quantizer handed the shared mask over un-materialised)
        if xa is None or self._attn_verify:
            with torch.enable_grad() if grad else contextlib.nullcontext():
                al = [t.detach().requires_grad_(grad) for t in (q4, k4, v4)]
                with self._ctx(S):
                    ao, _ = sdpa_attention_forward(self.attn, al[0], al[1], al[2], mask, dropout=0.0, scaling=scale)
                    ao = ao.reshape(B, S, -1).contiguous()
        if xa is not None:
            if ao is not None:          # the proof: torch's attention output beside the first-party one
                self._attn_diffs["out"] = self._attn_diffs.get("out", 0) + count_diff(xa[3].view(B, S, -1), ao.detach())
            a2d = xa[3].view(B * S, hq * hd)
        else:
            a2d = ao.detach().view(B * S, hq * hd)
        return a2d, (al, ao, xa)

    def _attention_backward(self, saved, da2d, B, S, scale, outs=None):
        """da2d [B * S, hq * hd] -> (gq4 [B, hq, S, hd], gk4, gv4 [B, hkv, S, hd]); outs: see `exact_attention_backward`"""
        al, ao, xa = saved
        if xa is None:
            return torch.autograd.grad(ao, al, da2d.view(B, S, -1))
        got = exact_attention_backward(xa, da2d.view(B, S, self.hq, self.hd), scale, outs=outs)
        if ao is not None:          # the proof: torch's gradients beside the first-party ones
            for name, mine, ref in zip(("dq", "dk", "dv"), got, torch.autograd.grad(ao, al, da2d.view(B, S, -1))):
                self._attn_diffs[name] = self._attn_diffs.get(name, 0) + count_diff(mine, ref)
        return got
