"""`StepDriver`: the step state machine under `nn.rollout.Rollout` and `partition.DistributedRollout`.

Before every step it decides whether the step runs eagerly, is captured into a hipGraph or is replayed, so that no replay reads packed
weights or per-mesh constants that changed since the capture; `validate()` reads the rollout's own range flags and, after a clip,
takes the steps again from the saved input window in "bf16x6".  A subclass fills `_one()` and `_warn_clipped()` and may override
`_capture()`, `_any_rank()`, `_restarted()` and `_rerun()`.  DESIGN.md §5 "The step driver" has the decision table."""
from __future__ import annotations

import torch

from . import ops, plan


class StepDriver:
    def _init_driver(self, field: torch.Tensor, out_steps, max_steps: int, capture) -> None:
        """`field`: the working input window (private to the rollout); `out_steps`: step-major [steps, rows, nf], or None."""
        self.field, self._out_steps, self.max_steps, self.capture = field, out_steps, int(max_steps), capture
        self.capture_error = None if capture else "capture not requested"
        self.step_counter = torch.zeros(2, dtype=torch.int32, device=field.device)     # [step index, g4c_rollout_advance's ticket]
        self.steps_done = 0
        self._hipgraph, self._epoch, self._pins = None, -1, None
        # per-mesh constants (the encoders of edge_attr / angle_attr*): computed by the first eager step, read by every later one
        self.static = ops.StaticCache()
        # fp16 range flags of this rollout's own launches: every step (eager, captured, recomputed) runs in their scope
        self.flags = ops.RangeFlags(field.device)
        # The default "f16x3" arithmetic is run OPTIMISTICALLY: its kernels flag every value that reached the end of the fp16 range
        # (|x| >= 65504, clipped there), `validate()` reads the flags, and a rollout that clipped anywhere is recomputed from the
        # window it started from in "bf16x6" (fp32's exponent range; the reference's `solve` runs in fp32, nn/model.py:303-321) and
        # stays in that arithmetic — so what is handed out never contains a clipped value.
        self._field0 = field.clone()             # the input window of slot `_first_slot`
        self._first_slot = 0
        self.exact_range = False                 # True once a clip made this rollout fall back to "bf16x6"

    # ---- hooks
    def _one(self) -> None:
        """The forward (inside `with self.static, self.flags`), then what closes the step."""
        raise NotImplementedError

    def _capture(self) -> None:
        torch.cuda.synchronize(self.field.device)
        self._pins = plan.snapshot()              # the graph bakes these pointers in: keep them past cache eviction
        hg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hg):                # records only; nothing executes during capture
            self._one()
        self._hipgraph = hg                       # (only now: a capture that raised leaves nothing behind to replay)
        hg.replay()

    def _any_rank(self, flag: bool) -> bool:
        """`flag` on any rank of the rollout (a collective every rank reaches); one rank here."""
        return flag

    def _warn_clipped(self, hit, n: int) -> None:
        """The RuntimeWarning of a clipped first pass (`hit`: this rank's MLPs that clipped, `n`: the steps taken again)."""
        raise NotImplementedError

    def _restarted(self, again: bool) -> None:
        """Steps are about to be taken anew from `_first_slot` (`again`: once more, because the first pass clipped)."""

    def _rerun(self, n: int) -> None:
        self.run(n)

    # ---- the driver
    @property
    def captured(self) -> bool:
        return self._hipgraph is not None

    @property
    def outputs(self) -> torch.Tensor:
        """[rows, nf * max_steps] as `GNN.solve` lays its result out (nn/model.py:322-326) — a fresh transposed copy of the step-major
        buffer on every access (no validation)."""
        return ops.steps_to_columns(self._out_steps)

    def step(self) -> None:
        if self.steps_done >= self.max_steps:
            raise RuntimeError(f"rollout buffer holds {self.max_steps} steps")
        if self.exact_range and ops.mlp_precision() == "f16x3":
            with ops.mlp_precision_as("bf16x6"):
                self._step()
        else:
            self._step()

    def _step(self) -> None:
        with torch.no_grad():
            if self._epoch != -1 and ops.weights_epoch() != self._epoch:
                # the weights changed since the last eager step (load_state_dict, fit, invalidate_packed; captured or not yet): the
                # packed images are stale or freed, and repacking (allocations + pack launches) must not happen inside a capture.
                # (Partitioned: every rank sees the same epoch sequence as long as every rank updates its replica of the model.)
                self._hipgraph, self._epoch = None, -1
            elif self.static.stale():
                # a per-mesh constant (edge_attr / angle_attr*) was edited in place, or the arithmetic changed: a captured step
                # contains neither the encoder launches nor a look-up of their cached results, and a step ABOUT to be captured
                #  would bake the recomputation — and, after a precision change, the repacking — into every replay.
                # (Partitioned: like new weights, something every rank has to do alike, or a replaying rank would pair its
                # captured collectives with an eager rank's.)
                self._hipgraph, self._epoch = None, -1
            if self.steps_done == 0 or not self.capture or self._epoch == -1:
                self._one()                               # eager: builds the plans and the packed weight images
                self._epoch = ops.weights_epoch()
            elif self._hipgraph is None:
                self._capture()
            else:
                self._hipgraph.replay()
        self.steps_done += 1

    def run(self, n: int) -> None:
        for _ in range(n):
            self.step()

    def validate(self) -> bool:
        """Default "f16x3" arithmetic: read the range flags of this rollout's launches (its own buffer, one synchronisation) and, if
        a value was clipped at the end of the fp16 range — on any rank —, take the steps `_first_slot .. steps_done` again from the
        saved input window in "bf16x6" (RuntimeWarning naming the MLPs); the rollout stays in that arithmetic.  Returns True when
        that happened.  (The early return depends on rank-uniform state only: every rank reaches `_any_rank`.)"""
        if ops.mlp_precision() != "f16x3" or self.exact_range:
            return False
        hit = self.flags.take()
        if not self._any_rank(bool(hit)):
            return False
        n = self.steps_done - self._first_slot
        self._warn_clipped(hit, n)
        self.exact_range = True
        self.field.copy_(self._field0)
        self.step_counter.zero_()
        if self._first_slot:
            self.step_counter[:1].fill_(self._first_slot)
        self._hipgraph, self._epoch = None, -1
        self.steps_done = self._first_slot
        self._restarted(True)
        self._rerun(n)
        return True
