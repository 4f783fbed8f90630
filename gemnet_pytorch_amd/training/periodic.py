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
those of `TrainStep`.  A new neighbour list every training step (padded or in-graph-rebuilt lists) is not provided.

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
targets, scale-factor fitting and the padded / in-graph runners in training mode still raise.
"""
import torch

from .ddp import TrainStep


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
