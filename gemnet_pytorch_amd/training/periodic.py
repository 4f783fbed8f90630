"""Training step for periodic batches (crystals, slabs, liquid boxes): `TrainStep` on a batch with a `cell`.

    builder = PeriodicGraphBuilder(N, cutoff, pbc=...)
    inputs = dict(Z=Z, R=R, N=N, cell=cell, **builder(R, cell))            # fixed index arrays
    ts = PeriodicTrainStep(model, rho_force=0.999, rho_stress=0.01, fused_optimizer=True)
    loss = ts(inputs, dict(E=Et, F=Ft, S=St))                              # or ts.capture(inputs, targets) first

The model runs its opt-in periodic training path (`GemNet.periodic_training`, model/gemnet.py: E, F, S with an autograd graph
to the parameters).  Loss:

    (1 - rho_force) mean|E - Et| + rho_force mean_a |F_a - Ft_a|_2 + rho_stress (1/B) sum_b |S_b - St_b|_F

with B the global structure count (all ranks); `targets["S"]` (B_local,3,3), dE/d(strain)/|det cell| in ASE's sign convention,
is needed only when rho_stress > 0.  Eager steps, `capture()`, the fused optimizer, the range flag and `world_size > 1` are
those of `TrainStep`.  A new neighbour list every training step — frames of a trajectory: new positions, a new cell and a new
image list each time — trains from ONE captured graph with `PeriodicPaddedTrainStep` (below): lists handed in and padded, or built
inside the replay.

A direct-force model (`GemNet(direct_forces=True)`, GemNet-dT) trains on the same batches: constructing the step opts the model
in (`periodic_direct_forces` and `periodic_training`), the model returns (E, F (A,1,3)) from its first-order training layers (chain programs with
trainable weights at the widths the chain kernel takes, else one launch per Dense) and the one-launch force head (`GemNet._forward_periodic_direct_train`, pbc.direct_forces_train), and the step is ONE first-order
backward.  Such a model has no stress: `rho_stress > 0` raises at construction.

    ts = PeriodicTrainStep(direct_model, rho_force=0.999, fused_optimizer=True)
    loss = ts(inputs, dict(E=Et, F=Ft))

GemNet-Q (`triplets_only=False`, forces by autograd) trains on the batches of `PeriodicQuadGraphBuilder`: constructing the step
opts the model in (`periodic_quadruplets`, `periodic_training` and `periodic_quadruplets_training`).  The second-order force graph
then runs on the edge vectors V and the interaction-edge vectors Vint (ops_train._AngleVec2Q / _QuadAnglesVec2,
csrc/pbc_quad_train.hip; pbc.force_stress_q); `rho_stress > 0` and `capture()` work as for GemNet-T.  A direct-force GemNet-Q, several
targets, scale-factor fitting (without `periodic_scale_fitting`) and the padded / in-graph runners in training mode still raise.

The scale factors themselves are fitted on periodic batches by `fit_scale_factors` (below): the loop of fit_scaling.py on a model
that opted in with `periodic_scale_fitting`, for GemNet-T, GemNet-dT and autograd-force GemNet-Q.
"""
import torch

from .ddp import USE_FUSED_LOSS, PaddedTrainStep, TrainStep, _PeriodicLoss


def fit_scale_factors(model, batches, num_batches=25, stress=False):
    """Fit every scale factor the model's scale file does not hold yet on periodic batches: the loop of fit_scaling.py:153-159.

        AutomaticFit.set2fitmode()
        model = GemNet(**cfg, scale_file=path).to("cuda")
        model.periodic_scale_fitting = True            # + the family's own switch (periodic_direct_forces / periodic_quadruplets)
        fitted = fit_scale_factors(model, batches)

    `batches`: a sequence (or any re-iterable) of periodic input dicts (Z, R, N, cell + the arrays of pbc.PeriodicGraphBuilder /
    PeriodicQuadGraphBuilder), cycled.  Per factor, in creation order: `num_batches` eval-mode calls, then its `fit()` (the one
    read-back of its statistic), which writes it to the scale file.  -> {name: value} as written.  On the way out — also after an
    error — fit mode is off and the schedule reset; the model is in eval mode and the next call runs the ordinary fused path
    with the fitted factors (the caches of derived weight forms are dropped)."""
    import itertools

    from ..model.scaling import AutomaticFit
    if not AutomaticFit.fitting_mode:
        raise RuntimeError("fit_scale_factors: build the model after AutomaticFit.set2fitmode()")
    if not getattr(model, "periodic_scale_fitting", False):
        raise RuntimeError("fit_scale_factors: opt the model in first (model.periodic_scale_fitting = True)")
    batches = list(batches) if not isinstance(batches, (list, tuple)) else batches
    if not batches or int(num_batches) < 1:
        raise ValueError("fit_scale_factors needs at least one batch and num_batches >= 1")
    fitted = {}
    model.eval()
    try:
        stream = itertools.cycle(batches)
        while not AutomaticFit.fitting_completed():
            for _ in range(int(num_batches)):
                model(next(stream), stress=stress)
            var = AutomaticFit.activeVar
            var.fit()
            fitted[var.name] = float(var.variable.detach().cpu())
    finally:
        AutomaticFit.fitting_mode = False
        AutomaticFit.reset()
        model._wcache = {}
        model._packs.clear()
    return fitted


class PeriodicTrainStep(TrainStep):
    def __init__(self, model, world_size=1, rho_force=0.999, grad_clip_max=10.0, optimizer=None, global_counts=None,
                 fused_optimizer=False, rho_stress=0.0):
        if getattr(model, "direct_forces", False) and float(rho_stress) > 0:
            raise ValueError("PeriodicTrainStep(rho_stress > 0): a direct-force model has no stress (its forces are not the "
                             "gradient of its energy); train it with rho_stress = 0")
        super().__init__(model, world_size=world_size, rho_force=rho_force, grad_clip_max=grad_clip_max, optimizer=optimizer,
                         global_counts=global_counts, fused_optimizer=fused_optimizer)
        self.rho_stress = float(rho_stress)
        if getattr(model, "direct_forces", False):
            model.periodic_direct_forces = True
        model.periodic_training = True
        if not getattr(model, "triplets_only", True) and not getattr(model, "direct_forces", False):
            model.periodic_quadruplets = True
            model.periodic_quadruplets_training = True
        self._S = None

    def _outputs(self, inputs):
        if inputs.get("cell") is None:
            raise ValueError("PeriodicTrainStep needs a periodic batch (inputs['cell']); use TrainStep for molecules")
        want_S = self.rho_stress > 0
        if self.flag is not None:
            inputs["_range_flag"] = self.flag        # for the duration of the call only (TrainStep._outputs)
        try:
            out = self.model(inputs, stress=want_S)
        finally:
            inputs.pop("_range_flag", None)
        self._S = out[2] if want_S else None
        E, F = out[0], out[1]
        if F.dim() == 3:          # a direct-force model: (A,1,3), as TrainStep._outputs
            F = F[:, 0]
        return E, F

    def loss(self, E, F, targets):
        B, A = self._counts(E.shape[0], F.shape[0], E.device)
        loss = self._energy_force_loss(E, F, targets, B, A)
        S, self._S = self._S, None
        if S is not None:
            # 9 B numbers: ATen
            d = (S - targets["S"].reshape(S.shape)).reshape(S.shape[0], 9)
            loss = loss + torch.linalg.vector_norm(d, dim=1).sum() * (self.rho_stress / B)
        return loss

    def _forward_backward(self, inputs, targets):
        if self.rho_stress > 0 and targets.get("S") is None:
            raise ValueError("PeriodicTrainStep(rho_stress > 0) needs the stress targets: targets['S'] of shape (B, 3, 3)")
        return super()._forward_backward(inputs, targets)


class PeriodicPaddedTrainStep(PaddedTrainStep):
    """`PeriodicTrainStep` for batches whose positions, cells, species and image neighbour lists change EVERY step (frames of a
    trajectory; the structure layout N is fixed), replayed from ONE captured hipGraph: `PaddedTrainStep` on a periodic
    `padded.PaddedGraphRunner` (the dummy molecule has a cell of its own, pad edges carry offset 0).  GemNet-T (E, F, S: the
    stress term with rho_stress > 0) and GemNet-dT (E, F); GemNet-Q and an atom capacity (`a_cap`) raise — the latter also for a model
    that sets `periodic_atom_capacity` (inference only: padded.PaddedGraphRunner).

        ts = PeriodicPaddedTrainStep(model, Z, N, e_cap, t_cap, cell=cell0, pbc=pbc, max_in_degree=deg, rho_stress=0.01,
                                     fused_optimizer=True)
        loss = ts.step(R, idx, cell, E_t, F_t, S_t)                       # idx: pbc.PeriodicGraphBuilder(N, cutoff)(R, cell)
        ts.attach_builder(pbc.PeriodicGraphBuilder(N, cutoff, pbc=pbc, device=dev))
        loss = ts.step_positions(R, cell, E_t, F_t, S_t)                  # the list is built inside the replay: no read-back

    The loss is `PeriodicTrainStep.loss` over the real structures (B = n_mol x world_size; the dummy molecule's energy, forces
    and stress row never enter it), with GEMNET_FUSED_LOSS=1 on the device one launch (kernels.periodic_loss).  The graph holds
    the optional index build, the index plan, the forward, the force graph, the loss and loss.backward(); the collective and
    the optimizer stay outside, as in `TrainStep`.

    A step of `step_positions` whose list outgrows the capacities (or breaks a padding rule: the error bits of
    gn_pbc_index_padded_t) ran on the previous step's arrays: its flat gradient and its loss are turned into NaN inside the
    graph, so the fused optimizer's non-finite check skips the update on the device (the eager optimizer reads the norm on the
    host and takes the same decision) — the parameters, the moments and Adam's step counter are those before the step.  The
    NEXT call raises ValueError with the capacities, the error bits and the sizes; the model stays in its arithmetic (no
    fall-back to the bf16 planes, no recapture).  The report is sticky: build a larger step.
    `world_size > 1` inherits `PaddedTrainStep`'s device-side exchange of the atom count; it has not been exercised."""

    # The capture runs on the warm-up's stream (TrainStep.CAPTURE_ON_WARMUP_STREAM).  On torch's capture stream the step of a
    # model on the composite closure (widths the chain kernel does not take) ended with "capturing stream has unjoined work" when
    # other captures had run in the process before: the warm-up's stream was drawn into the capture by gradient accumulators the
    # warm-up had left alive, and stayed unjoined.
    CAPTURE_ON_WARMUP_STREAM = True

    def __init__(self, model, Z, N, e_cap, t_cap, cell=None, pbc=None, max_in_degree=None, n_groups=None, rho_stress=0.0, **kw):
        if cell is None:
            raise ValueError("PeriodicPaddedTrainStep needs the structures' cells (cell=); use PaddedTrainStep for molecules")
        if not getattr(model, "triplets_only", True):
            raise NotImplementedError("PeriodicPaddedTrainStep: GemNet-T and GemNet-dT (triplets_only=True) only, not GemNet-Q "
                                      "(periodic GemNet-Q trains on fixed index arrays: PeriodicTrainStep)")
        if kw.get("a_cap") is not None and getattr(model, "periodic_atom_capacity", False):
            # (without the switch the runner's own refusal stands, word for word)
            raise NotImplementedError("PeriodicPaddedTrainStep: an atom capacity (a_cap) with a cell is served in inference only "
                                      "(padded.PaddedGraphRunner with model.periodic_atom_capacity); training keeps the fixed "
                                      "structure layout")
        direct = bool(getattr(model, "direct_forces", False))
        if direct and float(rho_stress) > 0:
            raise ValueError("PeriodicPaddedTrainStep(rho_stress > 0): a direct-force model has no stress (its forces are not the "
                             "gradient of its energy); train it with rho_stress = 0")
        super().__init__(model, Z, N, e_cap, t_cap, max_in_degree=max_in_degree, n_groups=n_groups, cell=cell, pbc=pbc, **kw)
        self.rho_stress = float(rho_stress)
        if direct:
            model.periodic_direct_forces = True
        model.periodic_training = True
        if self.rho_stress > 0:
            self.targets["S"] = torch.zeros(self.pad.n_mol, 3, 3, device=Z.device, dtype=self.targets["E"].dtype)
        self._S = None

    def attach_builder(self, builder):
        """From the next capture on the graph starts with the image neighbour list itself (PaddedGraphRunner.attach_builder:
        gn_pbc_index_padded_t reads positions AND cell at replay time).  The buffers must hold a first batch: one `step`, or
        `ts.pad._fill(R, idx, cell=cell)`."""
        self.pad.attach_builder(builder)
        self._graph = None
        self._captured = False
        self.inputs.pop("_plan", None)

    def _outputs(self, inputs):
        if not self._captured:
            inputs.pop("_plan", None)       # the plan is rebuilt INSIDE the capture from the static buffers (PaddedTrainStep)
        inputs["_guard_rows"] = (self.pad.n_mol, self.pad.a_cap)
        want_S = self.rho_stress > 0
        if self.flag is not None:
            inputs["_range_flag"] = self.flag
        try:
            out = self.model(inputs, stress=want_S)
        finally:
            inputs.pop("_range_flag", None)
        self._S = out[2][:self.pad.n_mol] if want_S else None
        E, F = out[0], out[1]
        if F.dim() == 3:          # a direct-force model: (A,1,3)
            F = F[:, 0]
        return E[:self.pad.n_mol], F[:self.pad.a_cap]

    def loss(self, E, F, targets):
        B = float(self.pad.n_mol * max(self.world_size, 1))
        S, self._S = self._S, None
        w_s = self.rho_stress / B
        if USE_FUSED_LOSS and E.is_cuda and E.dtype == torch.float32:
            return _PeriodicLoss.apply(E, F, S, targets["E"], targets["F"], targets["S"] if S is not None else None,
                                       (1 - self.rho) / (B * E.shape[1]), self.rho, w_s, self.mask, self.inv_atoms)
        loss = super().loss(E, F, targets)
        if S is not None:
            d = (S - targets["S"].reshape(S.shape)).reshape(S.shape[0], 9)
            loss = loss + torch.linalg.vector_norm(d, dim=1).sum() * w_s
        return loss

    def _in_graph(self):
        return self.pad.builder is not None and self.inputs["R"].is_cuda

    def _forward_backward(self, inputs, targets):
        if not self._in_graph():
            return super()._forward_backward(inputs, targets)
        from .. import kernels as K
        self.pad._index_in_graph()
        loss = super()._forward_backward(inputs, targets)
        # a list that did not fit: the step ran on the previous arrays.  force_loss / periodic_loss map a NaN difference to a
        # ZERO cotangent, so poisoned outputs would give a zero gradient and AdamW would still move the weights (momentum,
        # decay): the gradient itself and the loss are poisoned, the optimizer's non-finite check then skips the step
        K.index_poison(self.buf.flat, self.pad._idx_state)
        K.index_poison(loss, self.pad._idx_state)
        self.pad._idx_host.copy_(self.pad._idx_state, non_blocking=True)
        return loss

    def _index_overflow(self):
        err = self.pad.index_error() if self.pad.builder is not None else 0
        if err:
            raise ValueError(f"an earlier training step did not fit the capacities (e_cap {self.pad.e_cap}, t_cap {self.pad.t_cap}, "
                             f"in-degree bound {self.pad.pad_degree_bound()}): index error bits {err}, sizes "
                             f"{self.pad.index_sizes()} — the optimizer skipped it (the parameters did not move); build a larger "
                             "PeriodicPaddedTrainStep")

    def _check_index(self):
        """Start of every step: the report of the completed steps (pinned memory, no synchronisation unless it is set)."""
        if self.pad.builder is None or not self.pad.index_error():
            return
        torch.cuda.synchronize()
        self._range_check()         # a tripped flag (the optimizer skipped the step): corrects Adam's counter, resets, raises
        self._index_overflow()      # no optimizer step was asked for: nothing tripped, the report still stands

    def _need_stress_target(self, S_target):
        if self.rho_stress > 0 and S_target is None:
            raise ValueError("PeriodicPaddedTrainStep(rho_stress > 0) needs the stress targets: S_t of shape (n_mol, 3, 3)")

    def _load(self, cell, E_target, F_target, S_target):
        A = self.pad.A
        self.pad._set_cell(cell)
        self.targets["E"].copy_(E_target.reshape(self.targets["E"].shape))
        self.targets["F"][:A].copy_(F_target)
        self.mask[:A].fill_(1.0)
        if self.rho_stress > 0:
            self.targets["S"].copy_(S_target.reshape(self.targets["S"].shape))
        if self.world_size > 1:
            import torch.distributed as dist
            cnt = torch.full((), float(A), device=self.mask.device, dtype=torch.float64)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)          # device-side: no host sync, before the replay
            self.inv_atoms.copy_(1.0 / cnt)
        else:
            self.inv_atoms.fill_(1.0 / A)

    def _run(self, step_optimizer):
        if self.inputs["R"].is_cuda and not self._captured:
            self.capture(self.inputs, self.targets, check=getattr(self, "check", False))
            self._captured = True
        return self(self.inputs, self.targets, step_optimizer=step_optimizer)

    def step(self, R, idx, cell, E_target, F_target, S_target=None, Z=None, step_optimizer=True):
        """One training step on the lists handed in (pbc.PeriodicGraphBuilder's dict for R and cell)."""
        self._need_stress_target(S_target)
        self._check_index()
        self.pad._fill(R, idx, Z, None, cell)
        self._load(cell, E_target, F_target, S_target)
        return self._run(step_optimizer)

    def step_positions(self, R, cell, E_target, F_target, S_target=None, Z=None, step_optimizer=True):
        """One training step with the image neighbour list built inside the replay from R and cell: no host read-back."""
        if self.pad.builder is None:
            raise RuntimeError("step_positions needs attach_builder")
        if R.dtype != self.inputs["R"].dtype or tuple(R.shape) != (self.pad.A, 3):
            raise TypeError(f"step_positions: positions must be {self.inputs['R'].dtype} of shape ({self.pad.A}, 3); got "
                            f"{R.dtype} {tuple(R.shape)}")
        self._need_stress_target(S_target)
        self._check_index()
        if Z is not None:
            self.inputs["Z"][:self.pad.A].copy_(Z)
        self._load(cell, E_target, F_target, S_target)
        self.inputs["R"][:self.pad.A].copy_(R)
        return self._run(step_optimizer)
