"""The optimizer step in HIP, and the reference's learning-rate schedule.

``Adam`` is ``torch.optim.Adam`` with ``step()`` replaced by ``vqcpc_adam_step`` (``include/vqcpc.h``): one launch over all
tensors of a param group, in the one order of fp32 operations the header states.  Everything else -- ``state_dict()``,
``load_state_dict()``, ``param_groups``, ``state[p]`` (``step``, ``exp_avg``, ``exp_avg_sq``), ``zero_grad`` -- is torch's own, so a
state dict moves between the two optimizers in both directions, the ``"optimizer"`` entry of a reference checkpoint
(``train_cpc.py:17-33``) loads, and torch's schedulers drive ``group["lr"]`` unchanged.

``WarmupScheduler`` gives the learning rates of the reference's ``scheduler.py``: a linear ramp from ``initial_lr`` to ``max_lr``
over ``warmup_epochs`` epochs, then ``lr *= gamma`` at every milestone (``gamma ** k`` at one named k times).
"""
import collections

import torch

from . import _lib

try:
    from torch.optim.optimizer import _get_scalar_dtype
except ImportError:                                      # older torch: the step count of a state is a float32 scalar
    def _get_scalar_dtype():
        return torch.float32

_REJECTED = ("amsgrad", "maximize", "capturable", "differentiable")


def _name(group, i):
    """What a message calls parameter ``i`` of ``group``: its ``param_names`` entry where the group has them, else its position and shape."""
    names = group.get("param_names")
    p = group["params"][i]
    return f"parameter {names[i]!r}" if names else f"parameter {i} of the group (shape {tuple(p.shape)})"


class Adam(torch.optim.Adam):
    """``torch.optim.Adam`` whose ``step()`` is one ``vqcpc_adam_step`` call per param group, on the current stream of the
    parameters' device, over the parameters of the group that have a gradient, in group order.

    Plain Adam only: ``weight_decay != 0``, ``amsgrad``, ``maximize``, ``capturable`` and ``differentiable`` raise ``ValueError`` --
    here, and at ``step()`` for a group that ``add_param_group`` or ``load_state_dict`` brought in with one of them.  Parameters
    and gradients must be float32, dense and contiguous (``TypeError`` / ``ValueError`` at ``step()``, naming the tensor) and on the
    GPU (the project's ``no CPU fallback`` ``RuntimeError`` at ``step()``; construction and ``load_state_dict`` work on the CPU).

    ``state[p]["step"]`` counts per parameter as torch's does.  The entry takes one update number per call, so the parameters of a
    group that stand at different counts (one of them had no gradient for a while) go in one call per distinct count; a group
    whose parameters step together -- every fit of this project -- is one call.  The counts are mirrored on the host and read from
    ``state[p]["step"]`` again only when that tensor has been replaced (``load_state_dict``); the tensors themselves are 0-dim views
    into one buffer per group (values, dtype and device as torch's), so a group that steps together counts with one add.  ``step()`` bumps the parameters'
    ``_version`` as an in-place torch operator would, so the native handles see the new weights.

    What ``step()`` caches per parameter (its checks, its pointers, its count, its row of the group's table) is thrown away, for the
    whole group, when any of this has changed since the last step for a parameter that has a gradient: the parameter object at
    its position in ``group["params"]`` (a reorder, a replacement); the length of the group (``add_param_group`` aside, an append);
    the identity of ``state[p]["step"]``, ``["exp_avg"]`` or ``["exp_avg_sq"]`` (``load_state_dict``, also into an optimizer that
    has stepped; a state entry assigned by hand); ``data_ptr()`` of the parameter or of either moment (``p.data = ...``,
    ``.set_()``, ``.to()``).  The group then gets a NEW buffer of counts and every parameter's count is read from its
    ``state[p]["step"]`` before that tensor is rebound, so parameters that stand at different counts keep them through a reorder.
    Not looked at between steps: a value written into ``state[p]["step"]`` in place.  A parameter or moment that is not 16-byte
    aligned (a view that starts inside an allocation) is a ``ValueError`` naming it, before anything is written."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False, **kw):
        given = dict(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable)
        self._reject(given)
        if kw.get("fused") or kw.get("foreach"):
            raise ValueError("vectorquantizedcpc_amd.optim.Adam: foreach / fused choose among torch's own kernels; this step is vqcpc_adam_step")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, **kw)

    @staticmethod
    def _reject(group):
        if group.get("weight_decay", 0) != 0:
            raise ValueError(f"vectorquantizedcpc_amd.optim.Adam: weight_decay = {group['weight_decay']!r} is not supported (plain Adam only)")
        for k in _REJECTED:
            if group.get(k):
                raise ValueError(f"vectorquantizedcpc_amd.optim.Adam: {k} is not supported (plain Adam only)")

    def _check(self, group, i, t, what, like=None):
        """``TypeError`` / ``ValueError`` / ``RuntimeError`` naming the tensor if ``t`` (parameter ``i`` of ``group``, its gradient or
        a moment: ``what``) is not a dense, contiguous, 16-byte aligned float32 tensor on the GPU (of ``like``'s shape and device)."""
        who = what + _name(group, i)
        if t.layout is not torch.strided:
            raise TypeError(f"optim.Adam: {who} is {t.layout}, need a dense tensor")
        if t.dtype is not torch.float32:
            raise TypeError(f"optim.Adam: {who} is {t.dtype}, need torch.float32")
        if not t.is_cuda:
            raise RuntimeError(f"optim.Adam: {who} is on {t.device}: vectorquantizedcpc_amd runs on MI355X only; there is no CPU fallback")
        if not t.is_contiguous():
            raise ValueError(f"optim.Adam: {who} is not contiguous (strides {t.stride()} for shape {tuple(t.shape)})")
        if t.data_ptr() % 16:
            raise ValueError(f"optim.Adam: {who} is not 16-byte aligned (data_ptr() % 16 = {t.data_ptr() % 16}): vqcpc_adam_step reads "
                             "and writes 16-byte vectors, so a view that starts inside an allocation needs a copy of its own")
        if like is not None and (t.shape != like.shape or t.device != like.device):
            raise ValueError(f"optim.Adam: {who} has shape {tuple(t.shape)} on {t.device}, the parameter {tuple(like.shape)} on {like.device}")

    def _row(self, group, i, p, st, slots):
        """The cached row of parameter ``i`` of ``group``: the parameter and its state checked, the state made at its first update as
        torch makes it, the update count read from ``state[p]["step"]``, and row ``i`` of the group's table filled (all but the
        gradient).  ``state[p]["step"]`` becomes element ``i`` of the group's one buffer of counts (a 0-dim view, the value kept), so
        that a group that steps together counts with one add.  ``slots`` must be a buffer no live ``state[q]["step"]`` views yet
        (``step()`` makes a new one before it rebuilds a row): writing element ``i`` of a buffer in use would overwrite the count of
        the parameter that stood at ``i`` before.
        -> [p, step, count, exp_avg, exp_avg_sq, p's pointer, device, slots, i, exp_avg's pointer, exp_avg_sq's pointer]."""
        self._check(group, i, p, "")
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        m, v = st["exp_avg"], st["exp_avg_sq"]
        self._check(group, i, m, "state 'exp_avg' of ", p)
        self._check(group, i, v, "state 'exp_avg_sq' of ", p)
        counts, table = slots
        count = float(st["step"])
        st["step"] = counts[i]
        st["step"].fill_(count)
        t, at = table[i], (p.data_ptr(), m.data_ptr(), v.data_ptr())
        t.param, t.exp_avg, t.exp_avg_sq, t.numel = *at, p.numel()
        return [p, st["step"], int(round(count)), m, v, at[0], p.device, slots, i, at[1], at[2]]

    def _rows(self, group, slots, cache, fresh):
        """The rows of the parameters of ``group`` that have a gradient, by the number of the update they take, in group order, with
        the gradients' pointers written into the group's table.  A row is rebuilt (``_row``) when anything it cached has moved: the
        parameter object, its slot, the group's ``slots``, the identity of one of the three state tensors, or the storage
        (``data_ptr()``) of the parameter or of a moment.  Rows are rebuilt only into ``fresh`` slots; otherwise the first stale row
        ends the scan -> None, and ``step()`` scans again with new slots, which makes every row of the group stale."""
        params, state, table = group["params"], self.state, slots[1]
        f32, strided = torch.float32, torch.strided
        by_count = {}
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                continue
            st, row = state[p], cache.get(id(p))
            if (row is None or row[0] is not p or row[7] is not slots or row[8] != i or row[1] is not st.get("step")
                    or row[3] is not st.get("exp_avg") or row[4] is not st.get("exp_avg_sq") or row[5] != p.data_ptr()
                    or row[9] != row[3].data_ptr() or row[10] != row[4].data_ptr()):
                if not fresh:
                    return None
                row = cache[id(p)] = self._row(group, i, p, st, slots)
            if g.dtype is not f32 or g.layout is not strided or g.device != row[6] or not g.is_contiguous() or g.shape != p.shape:
                self._check(group, i, g, "the gradient of ", p)
            table[i].grad = g.data_ptr()
            count = row[2] + 1
            if count in by_count:
                by_count[count].append(row)
            else:
                by_count[count] = [row]
        return by_count

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cache = self.__dict__.setdefault("_hip_rows", {})        # id(p) -> _row: checked once, again when the parameter or its state moved
        groups = self.__dict__.setdefault("_hip_groups", {})     # group index -> (its buffer of counts, its table)
        for gi, group in enumerate(self.param_groups):
            self._reject(group)
            params = group["params"]
            slots = groups.get(gi)
            by_count = None
            if slots is not None and len(slots[1]) == len(params):
                by_count = self._rows(group, slots, cache, False)
            if by_count is None:                                 # the first step, another group length, or a stale row: new slots
                slots = groups[gi] = (torch.zeros(len(params), dtype=_get_scalar_dtype()), (_lib.AdamTensor * max(len(params), 1))())
                by_count = self._rows(group, slots, cache, True)
            table = slots[1]
            beta1, beta2 = group["betas"]
            for count, rows in by_count.items():
                n = len(rows)
                if n == len(params):                             # the whole group steps together: its table as it stands, one add
                    call, counts = table, slots[0]
                else:
                    call = self.__dict__.get("_hip_table")
                    if call is None or len(call) < n:
                        call = self.__dict__["_hip_table"] = (_lib.AdamTensor * n)()
                    for k, row in enumerate(rows):
                        call[k] = table[row[8]]
                    counts = None
                hyper = _lib.AdamHyper(float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), count)
                _lib.adam_step(call, n, hyper, rows[0][6])
                if counts is not None:
                    counts.add_(1)
                else:
                    torch._foreach_add_([row[1] for row in rows], 1)
                for row in rows:
                    row[2] = count
                torch.autograd.graph.increment_version([row[0] for row in rows])
        return loss


class WarmupScheduler(torch.optim.lr_scheduler.LRScheduler):
    """The learning rates of the reference's CPC trainer, one ``step()`` per epoch: at epoch ``e <= warmup_epochs`` the rate is
    ``initial_lr + (max_lr - initial_lr) * e / warmup_epochs``; after that it stays, and at an epoch that ``milestones`` names k
    times it is multiplied by ``gamma ** k``.  ``initial_lr`` and ``max_lr`` may be lists, one value per param group; they are kept
    in the groups (``group["initial_lr"]``, ``group["max_lr"]``) and so travel in the optimizer's state dict, the rest
    (``warmup_epochs``, ``milestones``, ``gamma``, ``last_epoch``) in this object's, under the names the reference's checkpoints
    use: its ``"scheduler"`` entry loads."""

    def __init__(self, optimizer, warmup_epochs, initial_lr, max_lr, milestones, gamma=0.1, last_epoch=-1):
        milestones = list(milestones)
        if not milestones or not warmup_epochs < min(milestones):
            raise ValueError(f"WarmupScheduler: the warm-up ({warmup_epochs} epochs) must end before the first milestone ({milestones})")
        if warmup_epochs < 0:
            raise ValueError(f"WarmupScheduler: warmup_epochs = {warmup_epochs}")
        self.warmup_epochs = warmup_epochs
        self.milestones = collections.Counter(milestones)
        self.gamma = gamma
        groups = optimizer.param_groups
        per_group = {}
        for name, value in (("initial_lr", initial_lr), ("max_lr", max_lr)):
            values = list(value) if isinstance(value, (list, tuple)) else [value] * len(groups)
            if len(values) != len(groups):
                raise ValueError(f"WarmupScheduler: {len(values)} values of {name} for {len(groups)} param groups")
            per_group[name] = values
        if last_epoch == -1:
            for i, group in enumerate(groups):
                group["initial_lr"], group["max_lr"] = per_group["initial_lr"][i], per_group["max_lr"][i]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        e, groups = self.last_epoch, self.optimizer.param_groups
        if e <= self.warmup_epochs:
            pct = e / self.warmup_epochs if self.warmup_epochs else 1.0
            return [(g["max_lr"] - g["initial_lr"]) * pct + g["initial_lr"] for g in groups]
        k = self.milestones.get(e, 0)
        if k == 0:
            return [g["lr"] for g in groups]
        return [g["lr"] * self.gamma ** k for g in groups]
