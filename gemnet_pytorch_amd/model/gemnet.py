"""`GemNet` — drop-in for the reference's `gemnet.model.gemnet.GemNet` (gemnet/model/gemnet.py:21-790)
with the InteractionBlock hot path running on hand-written gfx950 HIP kernels.

Kept verbatim from the reference: constructor signature (:82-113), `forward(inputs) -> (E, F)`
(:453-615; the force is differentiated w.r.t. a private leaf sharing `inputs["R"]`'s storage instead of toggling
`inputs["R"].requires_grad` :494,:613 — the caller's tensor is left untouched), `predict` (:780-784),
`load_weights`/`save_weights` (:786-790), attribute names the trainer reaches into
(`mlp_rbf3/.mlp_cbf3/.mlp_rbf_h/.mlp_rbf4/.mlp_cbf4/.mlp_sbf4/.mlp_rbf_out`, `num_blocks`,
`triplets_only`, `direct_forces`, trainer.py:263-278,417) and the state_dict key set.

Different by design: no zero-padded (E,Kmax,.) tensors, no `Kidx` host syncs, no sympy at
construction (closed-form basis kernels), no torch_scatter (CSR segmented sums), the concat-Dense
split into atom-side and edge-side GEMMs.  fp32 on a HIP device only; CPU tensors raise.

Force graph policy: the reference always builds the force with `create_graph=True`.  Here the
second-order graph is built when it can be used — `self.training and torch.is_grad_enabled()` —
or when `self.force_graph` is set to True/False explicitly.
"""
import contextlib
import math
import os

import torch

from .. import ops
from ..graph import GraphPlan
from .layers import (INV_SQRT_2, AtomEmbedding, BesselBasisLayer, Dense, EdgeEmbedding,
                     EfficientInteractionDownProjection, InteractionBlock,
                     InteractionBlockTripletsOnly, OutputBlock, SphericalBasisLayer, TensorBasisLayer)
from .scaling import AutomaticFit


_nullcontext = contextlib.nullcontext
_H3_GUARD = os.environ.get("GEMNET_H3_GUARD", "1") == "1"     # see GemNet.forward
# Side-stream placement switches.  All three were forced off in round 3 because hipGraph replays stopped matching the eager
# run with them; round 4 located the cause below the library — packed-FP32 instructions of the fused aggregation adjoint
# returning wrong lanes when its waves share CUs with the chain kernels of another graph branch (csrc/aggregate.hip,
# tools/exp/graph_corun.py, docs/HISTORY.md section 11) — and removed it, so they are on again.  `=0` restores the in-line forms.
_TRAIN_OVERLAP = os.environ.get("GEMNET_TRAIN_OVERLAP", "1") == "1"  # force training: output blocks on the side stream
_Q_OVERLAP = os.environ.get("GEMNET_Q_OVERLAP", "1") == "1"          # quadruplet models: output blocks on the side stream
_RBF_OUT_SIDE = os.environ.get("GEMNET_RBF_OUT_SIDE", "1") == "1"    # output-block radial projection in the forked head
_PLAN_LATE = os.environ.get("GEMNET_PLAN_LATE", "1") == "1"          # adjoint-only index structures on a stream of their own (in captures)


def K_chain_mode():
    from .. import kernels
    return kernels.current_mode()


class GemNet(torch.nn.Module):
    def __init__(
        self,
        num_spherical: int,
        num_radial: int,
        num_blocks: int,
        emb_size_atom: int,
        emb_size_edge: int,
        emb_size_trip: int,
        emb_size_quad: int,
        emb_size_rbf: int,
        emb_size_cbf: int,
        emb_size_sbf: int,
        emb_size_bil_quad: int,
        emb_size_bil_trip: int,
        num_before_skip: int,
        num_after_skip: int,
        num_concat: int,
        num_atom: int,
        triplets_only: bool,
        num_targets: int = 1,
        direct_forces: bool = False,
        cutoff: float = 5.0,
        int_cutoff: float = 10.0,
        envelope_exponent: int = 5,
        extensive=True,
        forces_coupled: bool = False,
        output_init="HeOrthogonal",
        activation: str = "swish",
        scale_file=None,
        name="gemnet",
        **kwargs,
    ):
        super().__init__()
        assert num_blocks > 0
        self.num_targets = num_targets
        self.num_blocks = num_blocks
        self.extensive = extensive
        self.forces_coupled = forces_coupled
        self.direct_forces = direct_forces
        self.triplets_only = triplets_only
        self.num_spherical = num_spherical
        self.force_graph = None  # None: auto (training & grad enabled); True/False: forced
        # opt-in: a periodic batch (inputs["cell"]) with a second-order force graph returns (E, F[, S]) with an autograd graph
        # to the parameters (_forward_periodic_train; training.periodic.PeriodicTrainStep sets it).  False: such a call raises
        self.periodic_training = False
        # opt-in: a direct-force model (`direct_forces=True`) serves periodic batches on the constant-weight inference path
        # (_forward_periodic_direct: no autograd, forces (A,1,3), no stress).  False: such a call raises
        self.periodic_direct_forces = False
        # opt-in: a GemNet-Q (`triplets_only=False`, forces by autograd) serves periodic batches in eval mode — the index arrays
        # of pbc.PeriodicQuadGraphBuilder, the quadruplet geometry on the edge and interaction-edge vectors (csrc/pbc_quad.hip):
        # (E, F[, S]).  False: such a call raises.  Training and direct forces with a cell stay GemNet-T only
        self.periodic_quadruplets = False
        # opt-in on top of `periodic_quadruplets`: the runners that follow a MOVING periodic system (padded.PaddedGraphRunner
        # with cell= and quad_caps=, runtime.DynamicForceField(cell=), md.DeviceMolecule / predict_periodic) accept this model —
        # the quadruplet index build inside the captured graph (csrc/pbc_index_qp.hip).  False: they raise as before
        self.periodic_quadruplets_dynamic = False
        # opt-in: scale-factor fitting (AutomaticFit.fitting_mode) on periodic batches, in eval mode, for GemNet-T, GemNet-dT
        # (with `periodic_direct_forces`) and GemNet-Q (with `periodic_quadruplets`): _forward_periodic_fit, driven by
        # training.periodic.fit_scale_factors.  False: a fit-mode call with a cell raises
        self.periodic_scale_fitting = False
        # arithmetic of the LDS-resident Dense stacks: None = the package default ("h3": fp32 operands as two fp16 planes,
        # three products), "split6" = three bf16 planes / six products (fp32 exponent range), "f32" = the f32-input MFMA — all
        # three at fp32 accuracy (force MAE 1e-6 .. 4e-6 eV/A against float64).  Single-plane bf16 / three-product modes exist
        # in the chain KERNEL (kernels.CHAIN_MODES, tests) but are not a model option: measured on the configs[4] shard they are
        # slower than the default (116 vs 109 ms) at 4e-2 eV/A (docs/HISTORY.md section 14)
        self.matmul_precision = None
        self.overlap_output_blocks = True
        self._side = None
        self._cot = None      # cached force cotangents (see _cotangent)
        self._wcache = {}  # derived (transposed / contiguous) copies of frozen weights, see ops.weight_cache
        self._packs = ops.PackRegistry()   # split-bf16 planes of the trainable weights, repacked once per training step

        AutomaticFit.reset()

        self.rbf_basis = BesselBasisLayer(num_radial, cutoff=cutoff, envelope_exponent=envelope_exponent)
        if not triplets_only:
            self.cbf_basis = SphericalBasisLayer(num_spherical, num_radial, cutoff=int_cutoff,
                                                 envelope_exponent=envelope_exponent, efficient=False)
            self.sbf_basis = TensorBasisLayer(num_spherical, num_radial, cutoff=cutoff,
                                              envelope_exponent=envelope_exponent, efficient=True)
        self.cbf_basis3 = SphericalBasisLayer(num_spherical, num_radial, cutoff=cutoff,
                                              envelope_exponent=envelope_exponent, efficient=True)

        # shared down projections (gemnet.py:158-204)
        if not triplets_only:
            self.mlp_rbf4 = Dense(num_radial, emb_size_rbf, activation=None, bias=False)
            self.mlp_cbf4 = Dense(num_radial * num_spherical, emb_size_cbf, activation=None, bias=False)
            self.mlp_sbf4 = EfficientInteractionDownProjection(num_spherical ** 2, num_radial, emb_size_sbf)
        self.mlp_rbf3 = Dense(num_radial, emb_size_rbf, activation=None, bias=False)
        self.mlp_cbf3 = EfficientInteractionDownProjection(num_spherical, num_radial, emb_size_cbf)
        self.mlp_rbf_h = Dense(num_radial, emb_size_rbf, activation=None, bias=False)
        self.mlp_rbf_out = Dense(num_radial, emb_size_rbf, activation=None, bias=False)

        self.atom_emb = AtomEmbedding(emb_size_atom)
        self.edge_emb = EdgeEmbedding(emb_size_atom, num_radial, emb_size_edge, activation=activation)

        block_cls = InteractionBlockTripletsOnly if triplets_only else InteractionBlock
        int_blocks = []
        for i in range(num_blocks):
            kw = dict(emb_size_atom=emb_size_atom, emb_size_edge=emb_size_edge, emb_size_trip=emb_size_trip,
                      emb_size_quad=emb_size_quad, emb_size_rbf=emb_size_rbf, emb_size_cbf=emb_size_cbf,
                      emb_size_bil_trip=emb_size_bil_trip, num_before_skip=num_before_skip,
                      num_after_skip=num_after_skip, num_concat=num_concat, num_atom=num_atom,
                      activation=activation, scale_file=scale_file, name=f"IntBlock_{i+1}")
            if not triplets_only:
                kw.update(emb_size_sbf=emb_size_sbf, emb_size_bil_quad=emb_size_bil_quad)
            int_blocks.append(block_cls(**kw))
        out_blocks = [
            OutputBlock(emb_size_atom=emb_size_atom, emb_size_edge=emb_size_edge, emb_size_rbf=emb_size_rbf,
                        nHidden=num_atom, num_targets=num_targets, activation=activation,
                        output_init=output_init, direct_forces=direct_forces, scale_file=scale_file,
                        name=f"OutBlock_{i}")
            for i in range(num_blocks + 1)
        ]
        self.out_blocks = torch.nn.ModuleList(out_blocks)
        self.int_blocks = torch.nn.ModuleList(int_blocks)

    # -------------------------------------------------------------------------- geometry (P9)
    @staticmethod
    def calculate_interatomic_vectors(R, id_s, id_t):
        """id_s / id_t: RowIndex of the source / target atoms (gemnet.py:261-286)."""
        V_st = ops.gather_rows(R, id_t) - ops.gather_rows(R, id_s)
        D_st = torch.sqrt(torch.sum(V_st ** 2, dim=1))
        return D_st, V_st / D_st[..., None]

    @staticmethod
    def calculate_neighbor_angles(R_ac, R_ab):
        """atan2(max(|u x v|, 1e-9), u.v)  (gemnet.py:288-311)."""
        x = torch.sum(R_ac * R_ab, dim=1)
        y = torch.linalg.cross(R_ac, R_ab, dim=-1).norm(dim=-1)
        y = torch.clamp(y, min=1e-9)
        return torch.atan2(y, x)

    @staticmethod
    def vector_rejection(R_ab, P_n):
        a_x_b = torch.sum(R_ab * P_n, dim=-1)
        b_x_b = torch.sum(P_n * P_n, dim=-1)
        return R_ab - (a_x_b / b_x_b)[:, None] * P_n

    @staticmethod
    def calculate_angles3(R, plan):
        """(gemnet.py:420-451) angle c<-a->b of every triplet."""
        Ra = ops.gather_rows(R, plan.t_a)
        R_ac = ops.gather_rows(R, plan.t_c) - Ra
        R_ab = ops.gather_rows(R, plan.t_b) - Ra
        return GemNet.calculate_neighbor_angles(R_ac, R_ab)

    REL_SIN2 = 1e-10        # kRelSin^2 of csrc/quad_math.h

    @staticmethod
    def quad_angles_of_vectors(uac, uab, ubd):
        """Phi_cab, Theta_cabd (Q,) of the quadruplets c -> a - b <- d from uac = c - a, uab = b - a, ubd = d - b (Q,3), in ATen
        and differentiable to any order — the composite closure of molecules (`calculate_angles`) and of periodic batches
        (`calculate_angles_vec`).  The clamp decisions are those of csrc/quad_math.h, relative to the vectors' lengths and taken
        on detached values: c - a - b collinear => Phi_cab is a constant; a vanished rejection => Theta_cabd = pi / 2, a
        constant; a planar quadruplet => Theta_cabd (0 or pi) is a constant."""
        rel2 = GemNet.REL_SIN2
        sq = lambda x: torch.sum(x * x, dim=-1)       # noqa: E731
        with torch.no_grad():
            p1, p2 = GemNet.vector_rejection(uac, uab), GemNet.vector_rejection(ubd, -uab)
            parallel = lambda u, v: sq(torch.linalg.cross(u, v, dim=-1)) <= rel2 * sq(u) * sq(v)       # noqa: E731
            flat = parallel(uab, uac)
            vanished = (sq(p1) <= rel2 * sq(uac)) | (sq(p2) <= rel2 * sq(ubd))
            fixed = (vanished | parallel(p1, p2))[:, None]
            flat = flat[:, None]
        angle_cab = GemNet.calculate_neighbor_angles(torch.where(flat, uab.detach(), uab), torch.where(flat, uac.detach(), uac))
        # (a row whose azimuth sits on its clamp sees detached vectors: the rejections carry no gradient there)
        tac, tab, tbd = (torch.where(fixed, x.detach(), x) for x in (uac, uab, ubd))
        angle_cabd = GemNet.calculate_neighbor_angles(GemNet.vector_rejection(tac, tab), GemNet.vector_rejection(tbd, -tab))
        angle_cabd = torch.where(vanished, torch.full_like(angle_cabd, math.pi / 2), angle_cabd)
        return angle_cab, angle_cabd

    @staticmethod
    def calculate_angles(R, plan):
        """Quadruplet angles (gemnet.py:334-418): Phi_cab (Q,), Phi_abd (I,), Theta_cabd (Q,).  The vectors are formed per
        intermediate triplet, as the reference forms them, and gathered to the quadruplets, where the two quadruplet angles
        take the decisions of `quad_angles_of_vectors` (an exactly planar or linear molecule in general orientation)."""
        q = plan.quad_geom
        Ra = ops.gather_rows(R, q["a_of_exp"])
        Rb = ops.gather_rows(R, q["b_of_exp"])
        Rd = ops.gather_rows(R, q["d_of_exp"])
        R_ba, R_bd = Ra - Rb, Rd - Rb
        angle_abd = GemNet.calculate_neighbor_angles(R_ba, R_bd)

        Rc = ops.gather_rows(R, q["c_of_red"])
        Ra2 = ops.gather_rows(R, q["a_of_red"])
        Rb2 = ops.gather_rows(R, q["b_of_red"])
        R_ac, R_ab = Rc - Ra2, Rb2 - Ra2
        angle_cab, angle_cabd = GemNet.quad_angles_of_vectors(ops.gather_rows(R_ac, q["reduce_cab"]),
                                                              ops.gather_rows(R_ab, q["reduce_cab"]),
                                                              ops.gather_rows(R_bd, plan.quad.expand))
        return angle_cab, angle_abd, angle_cabd

    @staticmethod
    def calculate_angles_vec(V, Vint, plan):
        """`calculate_angles` of a periodic batch on the edge vectors V (E,3) and the interaction-edge vectors Vint (n_int,3):
        Phi_cab (Q,), Phi_abd (I,), Theta_cabd (Q,) from uac = -V[ca], uab = -Vint[k], ubd = -V[db] per quadruplet and
        u = Vint[k], v = -V[db] per intermediate triplet (csrc/pbc_quad.hip)."""
        angle_abd = GemNet.calculate_neighbor_angles(ops.gather_rows(Vint, plan.intm_ab), -ops.gather_rows(V, plan.intm_db))
        uac = -ops.gather_rows(V, plan.quad.reduce)
        uab = -ops.gather_rows(ops.gather_rows(Vint, plan.intm_ab), plan.quad.expand)
        ubd = -ops.gather_rows(ops.gather_rows(V, plan.intm_db), plan.quad.expand)
        angle_cab, angle_cabd = GemNet.quad_angles_of_vectors(uac, uab, ubd)
        return angle_cab, angle_abd, angle_cabd

    # ---------------------------------------------------------------------------------- forward
    def _energy(self, R, plan, V=None, force_terms=False, Vint=None):
        """V: the (E,3) edge vectors of a periodic batch (pbc.edge_vectors; the leaf the force and stress are taken from).
        Vint: the (n_int,3) interaction-edge vectors of a periodic GemNet-Q batch (pbc.int_edge_vectors; the second leaf).
        `force_terms` (direct forces): return the output blocks' per-edge force terms as a list instead of their sum."""
        T = self.triplets_only
        b3 = self.cbf_basis3
        # Output blocks on a side stream (all model kinds, inference and force training; the round-3 restrictions are gone,
        # see the switches at the top of the file).
        overlap = self.overlap_output_blocks and (not ops.train2_enabled() or _TRAIN_OVERLAP)
        side = self._side_stream(R.device) if overlap and R.is_cuda and (T or _Q_OVERLAP) else None
        # The head of the forward is a string of small launches (110 us at B = 32); only distances -> edge embedding ->
        # rbf3 are needed by the first kernel of block 0.  With a side stream the rest forks off: the triplet angles,
        # the atom embedding and its two concat-Dense terms need positions / atomic numbers only and run beside the edge
        # geometry kernel; the circular-basis and the atom-update / output radial projections run beside the edge
        # embedding.  Autograd replays a node on its forward stream, so the tail of the backward overlaps the same way.
        # Triplets-only models only for now: the fork is measured (+2.5-3.8 %) and verified (graph replay == eager, bit
        # for bit) on GemNet-T; the quadruplet models spend 0.1 of 13.6 ms in this head and keep the sequential form.
        fork = side is not None and ops.is_fused() and T
        main = torch.cuda.current_stream(R.device) if fork else None
        h = terms = rbf_W1_3 = rbf_h = rbf_out = None
        # Fused radial head (ops.radial_head): the four radial projections leave the basis kernel, rad3 never exists, and
        # their adjoints, the sum of the rbf gradients and the basis adjoint are one launch.  GemNet-Q (needs rad3),
        # periodic batches, direct forces, trainable weights and other widths keep the launches below.
        proj = (self.mlp_rbf3, self.mlp_rbf_h, self.mlp_rbf_out)
        head = (ops.is_fused() and T and V is None and not self.direct_forces and R.is_cuda
                and all(d.bias is None and not d.act for d in proj)
                and ops.radial_head_supported(tuple(d.weight for d in proj) + (self.mlp_cbf3.weight,), b3.z_ln,
                                              self.rbf_basis.frequencies))
        # ... and the edge embedding with it (ops.radial_head_emb): its two atom terms are rows of tables over the 93
        # elements, so the two atom-row GEMMs, the K = 6 GEMM and its adjoint GEMM leave the step (GEMNET_RADIAL_EMB=0,
        # other widths, the f32 arithmetic: the launches below)
        ee = self.edge_emb
        emb = head and ops.radial_emb_supported(self.atom_emb.embeddings.weight, ee.dense.weight, ee.dense.act, ee.dense.bias,
                                                ee.atom_features)
        m = None
        if ops.is_fused():
            if fork:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    sph3 = ops.share_gradient(self._trip_basis3(R, plan, V))
                    h = self.atom_emb(plan.z_rows)
                    if not emb:
                        terms = self.edge_emb.atom_terms(h)
                    ev_a = torch.cuda.Event()
                    ev_a.record(side)
            # one launch: distances + Bessel rbf + spherical-Bessel radial basis; one launch: angles + Y_l0
            if V is not None:
                from .. import pbc
                D_ca, rbf, rad3 = pbc.edge_basis(V, self.rbf_basis.frequencies, b3.z_ln, b3.n_ln, b3.cutoff, b3.p)
                V_ca = None
            elif emb:
                m, rbf3, rbf_h, rbf_out, rbf_W1_3 = self._radial_head(R, plan, proj, emb=True)
                rbf = V_ca = None
            elif head:
                rbf, rbf3, rbf_h, rbf_out, rbf_W1_3 = self._radial_head(R, plan, proj)
                V_ca = None
            else:
                D_ca, V_ca, rbf, rad3 = ops.edge_basis(R, self.rbf_basis.frequencies, plan.id_c, plan.id_a,
                                                       b3.z_ln, b3.n_ln, b3.cutoff, b3.p,
                                                       want_V=self.direct_forces)
            if fork and head:
                # everything the side stream consumes of the head is rbf_out, and every output block orders itself behind
                # the main stream before it reads it (out_block below)
                main.wait_event(ev_a)
                for t in (sph3, h) + tuple(terms or ()):
                    t.record_stream(main)
            elif fork:
                ev_1 = torch.cuda.Event()
                ev_1.record(main)
                side.wait_event(ev_1)
                with torch.cuda.stream(side):
                    rbf.record_stream(side)
                    rad3.record_stream(side)
                    rbf_W1_3 = self.mlp_cbf3(rad3)
                    rbf_h = self.mlp_rbf_h(rbf)
                    if _RBF_OUT_SIDE:
                        rbf_out = self.mlp_rbf_out(rbf)
                    ev_b = torch.cuda.Event()
                    ev_b.record(side)
                # (all consumers of the output blocks' radial projection run on the side stream: so does the projection)
                if not _RBF_OUT_SIDE:
                    rbf_out = self.mlp_rbf_out(rbf)
                main.wait_event(ev_a)
                for t in (sph3, h) + tuple(terms):
                    t.record_stream(main)
            else:
                sph3 = ops.share_gradient(self._trip_basis3(R, plan, V))
        elif ops.train2_enabled() and not self.direct_forces:
            # force training: distances and triplet angles as twice-differentiable kernels (ops_train._Dist2 / _Angle2),
            # the bases on their closed derivative kernels
            from .. import ops_train
            if V is not None:     # periodic batch: the same pair of kernels on the edge vectors (_DistVec2 / _AngleVec2)
                D_ca, V_ca = ops_train.distances_vec(V), None
                angles = ops_train.triplet_angles_vec(V, plan.trip)
            else:
                D_ca, V_ca = ops_train.distances(R, plan.id_c, plan.id_a), None
                angles = ops_train.triplet_angles(R, plan.t_c, plan.t_a, plan.t_b)
            rbf = self.rbf_basis(D_ca)
            rad3, sph3 = b3(D_ca, angles)
        elif V is not None:
            # periodic batch on the composite closure (GEMNET_TRAIN2=0, matmul_precision="f32"): u = -V[reduce edge],
            # v = -V[expand edge], the image-aware c <- a -> b of pbc.trip_basis
            D_ca, V_ca = torch.sqrt(torch.sum(V ** 2, dim=1)), None
            rbf = self.rbf_basis(D_ca)
            rad3, sph3 = b3(D_ca, self.calculate_neighbor_angles(-ops.gather_rows(V, plan.trip.reduce),
                                                                 -ops.gather_rows(V, plan.trip.expand)))
        else:
            D_ca, V_ca = self.calculate_interatomic_vectors(R, plan.id_c, plan.id_a)
            rbf = self.rbf_basis(D_ca)
            rad3, sph3 = b3(D_ca, self.calculate_angles3(R, plan))
        cbf4_done = False       # (the fused branch below may project the circular basis through mlp_cbf4 itself)
        if not T and ops.is_fused():
            b4, qg = self.cbf_basis, plan.quad_geom
            # interaction-edge radial basis (cutoff = int_cutoff), a-b<-d angles and the quadruplet
            # harmonics, each one launch, straight from the positions
            if V is not None:
                # periodic batch: the same three launches on the vectors (csrc/pbc_quad.hip) — u = Vint, v = -V[d -> b] for
                # the a - b <- d angle; -V[c -> a], -Vint[a - b], -V[d -> b] for the quadruplet
                from .. import pbc
                rad4 = pbc.radial_basis(Vint, b4.z_ln, b4.n_ln, b4.cutoff, b4.p)
                y_abd = pbc.trip_basis2(Vint, V, plan, self.num_spherical)
            else:
                _, _, _, rad4 = ops.edge_basis(R, None, plan.int_b, plan.int_a, b4.z_ln, b4.n_ln, b4.cutoff, b4.p,
                                               want_rbf=False)
                y_abd = ops.trip_basis(R, qg["a_of_exp"], qg["b_of_exp"], qg["d_of_exp"], self.num_spherical)
            S, NR = self.num_spherical, b4.num_radial
            cbf4 = None
            if self.mlp_cbf4.bias is None and not self.mlp_cbf4.act:
                # gather + Hadamard with Y_l0 + mlp_cbf4 in one pass (csrc/cbf.hip); the projected basis is marked below
                cbf4 = ops.cbf_project(rad4, plan.intm_ab, y_abd, self.mlp_cbf4.weight)
            cbf4_done = cbf4 is not None
            if not cbf4_done:
                cbf4 = (ops.gather_rows(rad4, plan.intm_ab) * y_abd[:, :, None]).reshape(-1, S * NR)
            # (angle form for the published quadruplet widths: the bilinear kernels rebuild Y_lm from 16 B per quadruplet)
            ang = self.int_blocks[0].quad_interaction.mlp_sbf.weight.shape[:2] == (32, 32)
            if V is not None:
                sbf4 = (rad3, ops.share_gradient(pbc.quad_basis(V, Vint, plan, S, angle_form=ang)))
            else:
                sbf4 = (rad3, ops.share_gradient(ops.quad_basis(R, plan.q_c, plan.q_a, plan.q_b, plan.q_d, S, plan=plan,
                                                                angle_form=ang)))
        elif not T:
            qi = self.int_blocks[0].quad_interaction.mlp_sbf.weight
            if (ops.train2_enabled() and not self.direct_forces and self.num_spherical == 7
                    and ops.quad_train2_enabled(qi.shape[0], qi.shape[1], self.num_spherical ** 2)):
                # force training of the quadruplet interaction on fused kernels: the a - b <- d angles and the two quadruplet
                # angles as twice-differentiable kernels, the tensor basis in ANGLE form (16 B per quadruplet; the bilinear
                # twins rebuild Y_lm and its tangent in-kernel, ops_train._BilinearAng2) — no (Q, 49) array in any of the four
                # sweeps, no ATen launch over (Q, 3) temporaries
                from .. import ops_train
                if V is not None:
                    # periodic batch: the same three on the two vector arrays (csrc/pbc_quad_train.hip, ops_train._AngleVec2Q /
                    # _QuadAnglesVec2), the clamp decisions of the quadruplet angles relative to the vectors' lengths
                    D_ab = ops_train.distances_vec(Vint)
                    Phi_abd = ops_train.triplet_angles_vec2(Vint, V, plan)
                    ang = ops_train.quad_angles_vec(V, Vint, plan)
                else:
                    qg = plan.quad_geom
                    D_ab = ops_train.distances(R, plan.int_b, plan.int_a)
                    Phi_abd = ops_train.triplet_angles(R, qg["a_of_exp"], qg["b_of_exp"], qg["d_of_exp"])
                    ang = ops_train.quad_angles(R, plan.q_c, plan.q_a, plan.q_b, plan.q_d, plan)
                cbf4 = self.cbf_basis(D_ab, Phi_abd, plan.intm_ab)
                sbf4 = (rad3, ang)
            else:
                if V is not None:
                    # periodic batch on the composite closure (other widths, force_graph=True, GEMNET_TRAIN2=0, the quadruplet
                    # twins switched off, matmul_precision="f32"): ATen on (V, Vint), the A/B reference of the fused form
                    if ops.train2_enabled():
                        from .. import ops_train
                        D_ab = ops_train.distances_vec(Vint)
                    else:
                        D_ab = torch.sqrt(torch.sum(Vint ** 2, dim=1))
                    Phi_cab, Phi_abd, Theta_cabd = self.calculate_angles_vec(V, Vint, plan)
                else:
                    if ops.train2_enabled() and not self.direct_forces:
                        from .. import ops_train
                        D_ab = ops_train.distances(R, plan.int_b, plan.int_a)
                    else:
                        D_ab, _ = self.calculate_interatomic_vectors(R, plan.int_b, plan.int_a)
                    Phi_cab, Phi_abd, Theta_cabd = self.calculate_angles(R, plan)
                cbf4 = self.cbf_basis(D_ab, Phi_abd, plan.intm_ab)           # (I, S*R)
                # the tensor basis shares cutoff and radial tables with cbf_basis3: reuse rad3
                sbf4 = (rad3, ops.ylm(Phi_cab, Theta_cabd, self.num_spherical))  # ((E,S,R), (Q,S^2))

        if h is None:
            h = self.atom_emb(plan.z_rows)
        if m is None:
            rbf = ops.accumulate_gradient(rbf)
            m = self.edge_emb(h, rbf, plan.id_c, plan.id_a, terms=terms)

        if not T:
            rbf4 = ops.accumulate_gradient(self.mlp_rbf4(rbf))
            if not cbf4_done:
                cbf4 = self.mlp_cbf4(cbf4)
            cbf4 = ops.accumulate_gradient(cbf4)     # (one consumer per block: no engine-side (I,16) adds)
            sbf4 = (ops.accumulate_gradient(self.mlp_sbf4(sbf4[0])), sbf4[1])
        else:
            rbf4 = cbf4 = sbf4 = None
        # radial projections shared by all blocks: their gradients are summed inside the consumers' backward kernels
        rbf3 = ops.accumulate_gradient(rbf3 if head else self.mlp_rbf3(rbf))
        if head:
            cbf3 = (ops.accumulate_gradient(rbf_W1_3), sph3)
            rbf_h = ops.accumulate_gradient(rbf_h)
        elif fork:
            main.wait_event(ev_b)
            for t in (rbf_W1_3, rbf_h):    # produced on the side stream, consumed (and summed: `stream=`) on the main one
                t.record_stream(main)
            cbf3 = (ops.accumulate_gradient(rbf_W1_3, stream=main), sph3)
            rbf_h = ops.accumulate_gradient(rbf_h, stream=main)
        else:
            cbf3 = (ops.accumulate_gradient(self.mlp_cbf3(rad3)), sph3)
            rbf_h = ops.accumulate_gradient(self.mlp_rbf_h(rbf))
            rbf_out = self.mlp_rbf_out(rbf)

        # OutputBlock i only feeds the final energy sum.  Two forms:
        #  * grouped (`_out_group_blocks`: GemNet-T force pass with constant weights, the published widths, one target):
        #    all blocks run ONCE, in line, after the last interaction block, as three launches over (block, atom) tiles
        #    (ops.output_group: grouped aggregation, grouped chain launch, energy head) and three in the backward.  Per
        #    block the launches are latency-bound and fill a quarter of the CUs; on a side stream they were not free
        #    either (they slowed the main chain's kernels they ran beside, and the backward's five adjoint groups ran back
        #    to back in front of the main chain's first adjoint).  Deferring them UNGROUPED measured 4.5 % slower than
        #    the side stream: the grouping is the point.  Only the output blocks leave the side stream — the forked head
        #    above stays on it.
        #  * per block on a side stream (everything else), concurrently with InteractionBlock i+1 (and, since autograd
        #    replays a node on its forward stream, so does its backward).  Captured hipGraphs keep the fork/join as
        #    graph edges.
        outs = []
        # decided HERE, before the first interaction block: a pass that does not group keeps the interleaved issue below
        group = self._out_group_blocks(R, m, rbf_out)
        group_ms = []

        def ready():
            """Event on the main stream: (h, m) of this point exist.  None without a side stream."""
            if side is None:
                return None
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            return ev

        def out_block(i, h, m, ev):
            # the energies are summed along the chain of output blocks (epilogue of each energy head); the direct
            # force terms, when present, are summed below
            E_sum = outs[-1][0] if outs else None
            if side is None:
                outs.append(self.out_blocks[i](h, m, rbf_out, plan.id_a, E_sum=E_sum))
                return
            side.wait_event(ev)
            with torch.cuda.stream(side):
                for t in (h, m, rbf_out):
                    t.record_stream(side)
                outs.append(self.out_blocks[i](h, m, rbf_out, plan.id_a, E_sum=E_sum))

        # OutputBlock i is ISSUED after InteractionBlock i (it only waits for the event recorded before it): in a
        # captured hipGraph the first-captured successor of a fork keeps the queue, and with the output block issued
        # first the main chain changed queues at every block (10-17 us idle per hop, tools/timeline.py); the later
        # issue also gives the output block the higher autograd sequence number, so its backward is enqueued (on the
        # side stream) before the backward of the interaction block that needs its contribution to dE/dm.
        # (Issuing the output block of the LAST interaction block early — so that its backward is not enqueued between
        # the backward of output block nb, which the main chain waits for, and the main chain itself — measured 4 %
        # slower on the same box.)
        for i in range(self.num_blocks):
            ev = ready() if group is None else None
            h_i, m_i = h, m
            h, m = self.int_blocks[i](h=h, m=m, rbf4=rbf4, cbf4=cbf4, sbf4=sbf4, rbf3=rbf3, cbf3=cbf3,
                                      rbf_h=rbf_h, plan=plan)
            if group is None:
                out_block(i, h_i, m_i, ev)
            else:
                group_ms.append(m_i)
        if group is None:
            out_block(self.num_blocks, h, m, ready())
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        if group is not None:
            # every block's aggregation joins the running gradient of its m (ops.accumulate_gradient in the interaction
            # block that consumed it): the grouped adjoint runs first in the backward and seeds those sums
            if side is not None:
                rbf_out.record_stream(torch.cuda.current_stream())     # (produced on the side stream without the fused head)
            E_a, F_ca = ops.output_group(group, group_ms + [m], rbf_out, plan.id_a, s=INV_SQRT_2), 0
        else:
            E_a, F_ca = outs[-1][0], outs[0][1]
            if force_terms:
                F_ca = [F for _, F in outs]
                if side is not None:
                    for F in F_ca:       # produced on the side stream, consumed by the force head on this one
                        F.record_stream(torch.cuda.current_stream())
            else:
                for _, F in outs[1:]:
                    F_ca = F_ca + F

        E_mol = ops.segsum_rows(E_a, plan.batch_seg)                      # (nMolecules, num_targets)
        if not self.extensive:
            E_mol = E_mol / plan.atoms_per_mol.clamp(min=1)[:, None]
        return E_mol, F_ca, V_ca

    def _out_group_blocks(self, R, m, rbf_out):
        """The OutputBlocks in the form `ops.output_group` takes, or None when this pass keeps one set of launches per block:
        GemNet-Q, training (trainable weights / the twice-differentiable path), direct forces, scale fitting, several
        targets, host tensors, blocks that are not Dense + ResidualLayer stacks on the fused aggregation, and whatever
        `ops.output_group_supported` turns away (other widths, a chain arithmetic or kernel layout without the grouped launch,
        the aggregation switched off).  `m`: the edge embedding — every block's m has its shape."""
        if not (self.triplets_only and R.is_cuda and ops.is_fused() and ops.constant_weights() and not ops.train2_enabled()
                and not self.direct_forces and not AutomaticFit.fitting_mode and ops.USE_OUT_GROUP):
            return None
        blocks = []
        for ob in self.out_blocks:
            if not (ob.fuse_aggregate and not ob.direct_forces and ob.dense_rbf.bias is None and not ob.dense_rbf.act
                    and ob._stackable(ob.seq_energy) and ob.out_energy.bias is None and not ob.out_energy.act
                    and ob.out_energy.weight.shape[0] == 1):
                return None
            gemms = [ob.seq_energy[0].weight]
            for layer in ob.seq_energy[1:]:
                gemms += [layer.dense_mlp[0].weight, layer.dense_mlp[1].weight]
            blocks.append(dict(W_rbf=ob.dense_rbf.weight, scale=ob.scale_sum.scale_factor, gemms=gemms,
                               act0=bool(ob.seq_energy[0].act), w_out=ob.out_energy.weight))
        return blocks if ops.output_group_supported(blocks, [m] * len(blocks), rbf_out) else None

    def _radial_head(self, R, plan, proj, emb=False):
        b3 = self.cbf_basis3
        if emb:
            return ops.radial_head_emb(R, self.rbf_basis.frequencies, plan.id_c, plan.id_a, b3.z_ln, b3.n_ln,
                                       tuple(d.weight for d in proj) + (self.mlp_cbf3.weight,), b3.cutoff, b3.p, plan.z_rows,
                                       self.atom_emb.embeddings.weight, self.edge_emb.dense.weight, self.edge_emb.atom_features)
        return ops.radial_head(R, self.rbf_basis.frequencies, plan.id_c, plan.id_a, b3.z_ln, b3.n_ln,
                               tuple(d.weight for d in proj) + (self.mlp_cbf3.weight,), b3.cutoff, b3.p)

    def _trip_basis3(self, R, plan, V):
        if V is not None:
            from .. import pbc
            return pbc.trip_basis(V, plan.trip, self.num_spherical)
        return ops.trip_basis(R, plan.t_c, plan.t_a, plan.t_b, self.num_spherical)

    def forward(self, inputs, stress=False):
        """E, F as the reference's `GemNet.forward` (gemnet.py:453-615).
        Periodic batches (`cell` (B,3,3) + `cell_offsets` (E,3), pbc.py; GemNet-T, eval-mode forces by autograd): the edge
        vectors carry the image shift; `stress=True` returns (E, F, S) with S (B,3,3) = dE/d(strain) / |det cell| (eV/A^3).
        A direct-force model (`direct_forces=True`) serves periodic batches with `periodic_direct_forces = True` (opt-in): (E, F)
        with F (A,1,3) as on molecules, no stress (`stress=True` raises); without the switch it raises.  Eval mode: no autograd.
        Training mode needs `periodic_training = True` as well (else it raises) and returns (E, F) with a first-order autograd
        graph to the parameters (`_forward_periodic_direct_train`).
        With `periodic_training = True` a call that builds the second-order force graph (training mode with grad enabled, or
        `force_graph = True`) returns the same outputs with an autograd graph to the parameters; without it that call raises.
        A GemNet-Q (`triplets_only=False`) needs `periodic_quadruplets = True` for a cell at all and, for that second-order graph,
        `periodic_quadruplets_training = True` as well (training.periodic.PeriodicTrainStep sets all three); else it raises.
        While the scale factors are being fitted (`AutomaticFit.fitting_mode`) a periodic batch needs `periodic_scale_fitting = True`
        and eval mode (`_forward_periodic_fit`, training.periodic.fit_scale_factors); else it raises.
        Range guard of the default Dense arithmetic: the "h3" forward programs keep activations in two fp16 planes, so a
        value beyond 65 504 becomes inf — fitted scale factors keep activations O(1), a model with
        unfitted ones (the starting state of fit_scaling.py, foreign checkpoints) need not.  A non-finite result of an eager
        forward in that arithmetic switches THIS model to the bf16-plane form ("split6": fp32 exponent range), says so, and
        repeats the pass.  (One host read-back per eager forward.  A hipGraph cannot read back: a runner hands its
        `runtime.RangeFlag` in as `inputs["_range_flag"]`, the captured pass ends with the device-side check of the same rows,
        and the runner polls the flag — PaddedGraphRunner, DynamicForceField, ForceGraphs, TrainStep.)"""
        periodic = inputs.get("cell") is not None
        if stress and not periodic:
            raise ValueError("stress=True needs a periodic batch (inputs['cell'])")
        if periodic and "cell_offsets" not in inputs:
            raise ValueError("a periodic batch needs its neighbour list with 'cell_offsets' (pbc.PeriodicGraphBuilder)")
        inputs = self.with_indices(inputs)
        with ops.exclusive():
            out = self._forward_guarded(inputs, stress)
        return out if (stress or not periodic) else out[:2]

    def with_indices(self, inputs):
        """`inputs` with the index arrays: as given when it has them, else (a `DataContainer(indices="device")` batch: Z, R, N
        on the device) a new dict with the arrays built on the GPU (index_device.ensure_indices).  Callers that CAPTURE a step
        call this first: the build reads sizes back, which a stream capture does not allow."""
        if "id_c" in inputs:
            return inputs
        from ..index_device import ensure_indices
        self._check_inputs(inputs["R"])
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("inputs without index arrays inside a stream capture: call model.with_indices(inputs) first")
        cutoff, int_cutoff = self.cbf_basis3.cutoff, getattr(getattr(self, "cbf_basis", None), "cutoff", 10.0)
        if "cutoffs" in inputs:     # DataContainer(indices="device"): the container's own cutoffs define the graph
            c = inputs["cutoffs"].detach().cpu().tolist()
            cutoff, int_cutoff = float(c[0]), float(c[1])
        return ensure_indices(inputs, cutoff, int_cutoff, self.triplets_only)

    def _forward_guarded(self, inputs, stress=False):
        out = self._forward(inputs, stress)
        R = inputs["R"]
        h3 = R.is_cuda and (self.matmul_precision or K_chain_mode()) == "h3"
        # (a padded batch — padded.py — names its real rows: the dummy molecule behind them is not the model's concern)
        rows = inputs.get("_guard_rows")
        flag = inputs.get("_range_flag")
        if flag is not None and R.is_cuda:
            # a runner's device-side range check (runtime.RangeFlag): two tiny launches + a copy of one word to pinned host
            # memory at the end of the pass — what a REPLAYED graph has instead of the read-back below
            E, F = out[0], out[1]
            flag.watch(E.detach()[:rows[0]] if rows is not None else E.detach(),
                       F.detach()[:rows[1]] if rows is not None else F.detach())
        if _H3_GUARD and h3 and not torch.cuda.is_current_stream_capturing():
            seen = out if rows is None else (out[0][:rows[0]], out[1][:rows[1]])
            if not bool(torch.stack([torch.isfinite(t).all() for t in seen]).all()):
                import warnings
                warnings.warn("gemnet_pytorch_amd: non-finite energies / forces from the fp16-plane Dense arithmetic ('h3': "
                              "activations beyond 65504 overflow; are the scale factors fitted?) — this model now uses "
                              "matmul_precision = 'split6' (bf16 planes, fp32 range); the pass is repeated", RuntimeWarning)
                self.matmul_precision = "split6"
                self._wcache = {}
                if getattr(self, "_packs", None) is not None:
                    self._packs.clear()
                if flag is not None:
                    torch.cuda.current_stream().synchronize()
                    flag.reset()       # the eager pass reported it itself
                out = self._forward(inputs, stress)
        return out

    PRECISIONS = (None, "h3", "split6", "f32")

    def _forward(self, inputs, stress=False):
        R = inputs["R"]
        self._check_inputs(R)
        if self.matmul_precision not in self.PRECISIONS and not getattr(self, "_experimental_precision", False):
            raise ValueError(f"matmul_precision must be one of {self.PRECISIONS}; got {self.matmul_precision!r} (reduced-precision "
                             "operand modes are kernel-level experiments, not a model option: slower AND 4e-2 eV/A off on "
                             "BASELINE configs[4], docs/HISTORY.md section 14)")
        cell = inputs.get("cell")
        if cell is not None:
            self._check_periodic(inputs, stress)
        plan = GraphPlan.from_inputs(inputs, self.triplets_only)
        late = None
        pos_graph = False
        if R.is_cuda and self.overlap_output_blocks:
            # the output blocks run on a side stream: every lazily-built index structure they share with the main
            # stream (CSR sorts, triplet groups) must exist before the fork, not be built by whichever stream gets
            # there first (an un-warmed GemNet-Q batch aborted with a memory fault in one of three runs).
            # A plan that is built INSIDE a capture (padded.py: rebuilt by every replay) puts the structures that only the
            # adjoint kernels read — two sorts of T keys among them — on a stream of their own, beside the forward pass.
            if (_PLAN_LATE and self.triplets_only and not self.direct_forces and not getattr(plan, "_warmed", False)
                    and torch.cuda.is_current_stream_capturing()):
                late = self._side_stream(R.device, "plan")
            plan.warm(late_stream=late)
        if not self.direct_forces:
            # The reference flips `inputs["R"].requires_grad` on the caller's tensor (gemnet.py:494,:613).  Here the
            # force is differentiated w.r.t. a FRESH leaf that shares R's storage: autograd keeps a leaf's gradient
            # accumulator — tied to the stream of its first backward — on the tensor object, and positions that once
            # went through a forward on the default stream made later hipGraph captures of the same batch fail
            # (the engine synchronised the capturing stream with the default stream).
            # A caller whose R already takes part in an autograd graph (a non-leaf, or a leaf that requires grad:
            # Hessians, position-dependent losses) keeps its tensor, as in the reference.
            if R.requires_grad:
                pos_graph = True      # the caller may differentiate through the force w.r.t. its positions (ops.position_graph)
            else:
                R = R.detach().requires_grad_(True)
        # second-order graph only when it can be used (see module docstring)
        graph = self.force_graph
        if graph is None:
            graph = self.training and torch.is_grad_enabled() and not self.direct_forces
        # fused single-launch layers whenever no double backward will run through them; the
        # scale-factor fitting mode needs the unfused layer order to observe variances
        fused = not graph and not AutomaticFit.fitting_mode

        # force-by-autograd without a second-order graph: the graph of E is consumed right here, so
        # parameter gradients can never be requested -> weights are constants (enables ops.stack)
        const_w = fused and not self.direct_forces
        # force training: the Dense stacks as twice-differentiable single-launch Functions (ops_train.py), the rest on
        # the composite closure; the split-operand chain kernel only (its f32 sibling has no second-order source terms)
        mode = self.matmul_precision or K_chain_mode()
        # (one target: with several, each target's force pass would need its own record of the S2 / S3 sweeps per stack and
        #  one source term per target in S4 — those models train on the composite closure)
        # (and widths the split-operand chain kernel takes in every sweep, see _train2_widths_ok: the CPU emulation takes any)
        t2 = (bool(graph) and ops.USE_TRAIN2 and not AutomaticFit.fitting_mode and mode != "f32" and self.num_targets == 1
              and (not R.is_cuda or self._train2_widths_ok()))
        if cell is not None and AutomaticFit.fitting_mode:
            # (`periodic_scale_fitting`, eval mode, fixed index arrays, no capture: _check_periodic turned the rest away)
            return self._forward_periodic_fit(R, plan, cell)
        if cell is not None and self.direct_forces:
            # (training mode: `periodic_training` is on — _check_periodic turned the rest away; eval mode never looks at it)
            if self.training:
                return self._forward_periodic_direct_train(R, plan, cell)
            return self._forward_periodic_direct(R, plan, cell)
        if cell is not None:
            if graph and not getattr(self, "periodic_training", False):
                raise NotImplementedError("periodic cells: forces by autograd on the first-order (eval) path only; training "
                                          "with a cell (a second-order force graph) is opt-in: set "
                                          "model.periodic_training = True (training.periodic.PeriodicTrainStep does)")
            out = self._forward_periodic_train(R, plan, cell, t2) if graph else self._forward_periodic(R, plan, cell)
            if late is not None:
                plan.join_late()
            return out
        with ops.weight_cache(self._wcache), ops.fused_first_order(fused), ops.param_grads(not const_w), \
                ops.train2(t2, self._packs if (t2 and R.is_cuda) else None), \
                ops.chain_mode(self.matmul_precision), ops.position_graph(pos_graph), \
                torch.enable_grad() if not self.direct_forces else _nullcontext():
            E_mol, F_ca, V_ca = self._energy(R, plan)

            if self.direct_forces:
                if self.forces_coupled:  # enforce |F_ac| = |F_ca| (gemnet.py:588-592)
                    F_ca = ops.segsum_rows(F_ca, plan.id_undir) * 0.5
                    F_ca = ops.gather_rows(F_ca, plan.id_undir)
                F_ji = F_ca[:, :, None] * V_ca[:, None, :]
                F_j = ops.segsum_rows(F_ji, plan.id_a)                         # (nAtoms, num_targets, 3)
            else:
                with ops.param_grads(False):  # only dE/dR is needed here
                    # F = -d(sum_mol E)/dR: the cotangent -1 (one column per target) goes in directly — no reduction,
                    # no ones_like fill and no negation launch
                    if self.num_targets > 1:
                        F_j = torch.stack(
                            [torch.autograd.grad(E_mol, R, grad_outputs=self._cotangent(E_mol, i), create_graph=graph,
                                                 retain_graph=True)[0] for i in range(self.num_targets)], dim=1)
                    else:
                        F_j = torch.autograd.grad(E_mol, R, grad_outputs=self._cotangent(E_mol, 0),
                                                  create_graph=graph)[0]
        if late is not None:
            plan.join_late()
        return E_mol, F_j

    def _train2_widths_ok(self):
        """The adjoint and tangent sweeps of the fused training form are GEMMs whose N is an embedding width: the split-operand
        chain kernel takes multiples of 16 (kernels.chain_split_supported) and its f32 sibling carries no second-order source
        terms, so a model with another embedding width (test-sized models: 8-wide radial / triplet embeddings) trains on the
        composite closure as a whole."""
        b = self.int_blocks[0]
        t = b.trip_interaction
        widths = [self.atom_emb.embeddings.weight.shape[1], self.mlp_rbf3.weight.shape[0], self.mlp_cbf3.weight.shape[2],
                  *t.down_projection.weight.shape, t.up_projection_ca.weight.shape[1]]
        if not self.triplets_only:
            q = b.quad_interaction
            widths += [self.mlp_rbf4.weight.shape[0], self.mlp_cbf4.weight.shape[0], self.mlp_sbf4.weight.shape[2],
                       q.down_projection.weight.shape[0], q.up_projection_ca.weight.shape[1]]
        return all(int(w) % 16 == 0 for w in widths)

    def _check_periodic(self, inputs, stress=False):
        """What a cell is not supported with raises (no silent molecular result)."""
        who = "periodic cells" if self.triplets_only else "periodic cells (GemNet-Q)"
        if AutomaticFit.fitting_mode and getattr(self, "periodic_scale_fitting", False):
            # scale-factor fitting with a cell (opt-in): one eval-mode pass over fixed index arrays per batch, outside a capture
            # (AutoScaleFit counts rows on the host and fit() reads the sums back) — the rest of this method judges the family
            if self.training or self.force_graph:
                raise NotImplementedError(f"{who}: scale-factor fitting with a cell runs in eval mode without a force graph "
                                          "(model.eval(), force_graph = None)")
            if inputs.get("_guard_rows") is not None:
                raise NotImplementedError(f"{who}: scale-factor fitting with a cell runs on fixed index arrays only — the dummy "
                                          "rows of a padded batch would enter the statistics")
            if inputs["R"].is_cuda and torch.cuda.is_current_stream_capturing():
                raise NotImplementedError(f"{who}: scale-factor fitting with a cell cannot run inside a stream capture")
        if not self.triplets_only:
            if not getattr(self, "periodic_quadruplets", False):
                raise NotImplementedError("periodic cells: GemNet-T (triplets_only=True) only, not GemNet-Q (eval-mode GemNet-Q "
                                          "is opt-in: model.periodic_quadruplets = True, pbc.PeriodicQuadGraphBuilder)")
            if self.direct_forces:
                raise NotImplementedError("periodic cells: a direct-force GemNet-Q is not served with a cell")
            graph = self.force_graph
            if graph is None:
                graph = self.training and torch.is_grad_enabled()
            # (training — the second-order force graph on (V, Vint) — is a third opt-in, `periodic_quadruplets_training`, on top
            #  of `periodic_training`; training.periodic.PeriodicTrainStep sets all three)
            if graph and not getattr(self, "periodic_quadruplets_training", False):
                raise NotImplementedError("periodic cells: GemNet-Q runs on the first-order (eval) path only; training with a "
                                          "cell is GemNet-T only")
            if graph and inputs.get("_guard_rows") is not None:
                raise NotImplementedError("periodic cells (GemNet-Q): training runs on fixed index arrays only, not on the "
                                          "padded or in-graph-rebuilt lists of padded.PaddedGraphRunner")
            if "int_cell_offsets" not in inputs:
                raise ValueError("a periodic GemNet-Q batch needs 'int_cell_offsets' and the quadruplet arrays of "
                                 "pbc.PeriodicQuadGraphBuilder")
        if self.direct_forces:
            if not getattr(self, "periodic_direct_forces", False):
                raise NotImplementedError("periodic cells: forces by autograd only, not direct_forces")
            if self.training and not getattr(self, "periodic_training", False):
                raise NotImplementedError("periodic cells: direct-force periodic batches are inference only (model.eval())")
            if stress:
                raise NotImplementedError("periodic cells: a direct-force model has no stress (its forces are not the "
                                          "gradient of its energy)")
        # (the messages of a quadruplet model name it: every refusal of a periodic GemNet-Q batch says "GemNet-Q")
        if self.num_targets != 1:
            raise NotImplementedError(f"{who}: one target only")
        if AutomaticFit.fitting_mode and not getattr(self, "periodic_scale_fitting", False):
            raise NotImplementedError(f"{who}: no scale-factor fitting with a cell")
        # (padded batches — padded.PaddedGraphRunner(cell=...) — are ordinary periodic batches: the dummy molecule has a cell
        #  row of its own and its pad edges carry offset 0; `_guard_rows` / `max_in_degree` mean what they mean for molecules)
        if inputs["R"].requires_grad:
            raise NotImplementedError(f"{who}: positions that take part in an autograd graph are not supported")

    def _forward_periodic(self, R, plan, cell):
        """E, F, S of a periodic batch.  Everything depends on R through the edge vectors V (the shift is constant), so the
        force and the stress come from ONE gradient, G = -dE/dV per edge: F = segsum(G, id_a) - segsum(G, id_c) and
        S_b = -1/|det cell_b| sum_{e of b} V_e (x) G_e."""
        from .. import pbc
        V = pbc.edge_vectors(R, plan, cell).requires_grad_(True)
        # GemNet-Q (`periodic_quadruplets`): a second leaf, the interaction-edge vectors Vint — the quadruplet geometry needs
        # exactly V and Vint — and the same ONE gradient call: F and S add the interaction edges' terms
        Vint = None if self.triplets_only else pbc.int_edge_vectors(R, plan, cell).requires_grad_(True)
        with ops.weight_cache(self._wcache), ops.fused_first_order(True), ops.param_grads(False), \
                ops.train2(False, None), ops.chain_mode(self.matmul_precision), ops.position_graph(False), \
                torch.enable_grad():
            E_mol, _, _ = self._energy(R.detach(), plan, V=V, Vint=Vint)
            if Vint is None:
                G = torch.autograd.grad(E_mol, V, grad_outputs=self._cotangent(E_mol, 0))[0]
            else:
                G, Gint = torch.autograd.grad(E_mol, (V, Vint), grad_outputs=self._cotangent(E_mol, 0), allow_unused=True)
        if Vint is None:
            F = pbc.forces(G, plan)
            S = pbc.stress(V.detach(), G, plan, cell)
        else:
            G = torch.zeros_like(V) if G is None else G
            Gint = torch.zeros_like(Vint) if Gint is None else Gint
            F = pbc.forces_q(G, Gint, plan)
            S = pbc.stress_q(V.detach(), G, Vint.detach(), Gint, plan, cell)
        return E_mol.detach(), F, S

    def _forward_periodic_fit(self, R, plan, cell):
        """The eval call's outputs — (E, F, S), or (E, F (A,1,3)) from a direct-force model — of a periodic batch while the scale
        factors are being fitted (`periodic_scale_fitting`): the UNFUSED layer order on the edge vectors V (and Vint), the one the
        factors' observation points sit in (`_forward_periodic_train`'s order), with constant weights and a first-order force
        gradient only.  Inside `scaling.periodic_statistic()` the two bilinear sums hand their expand index to the factor and the
        active factor takes the device statistic (gn_col_var_f32; GEMNET_FIT_STAT=0: a materialised gather + torch.var)."""
        from .. import pbc
        from .scaling import periodic_statistic
        ctx = (ops.weight_cache(self._wcache), ops.fused_first_order(False), ops.param_grads(False), ops.train2(False, None),
               ops.chain_mode(self.matmul_precision), ops.position_graph(False), periodic_statistic(True))
        with contextlib.ExitStack() as stack:
            for c in ctx:
                stack.enter_context(c)
            if self.direct_forces:
                V = pbc.edge_vectors(R, plan, cell)
                with torch.no_grad():
                    E_mol, terms, _ = self._energy(R.detach(), plan, V=V, force_terms=True)
                    F = pbc.direct_forces(torch.stack(terms), V, plan, self.forces_coupled)
                return E_mol, F
            V = pbc.edge_vectors(R, plan, cell).requires_grad_(True)
            Vint = None if self.triplets_only else pbc.int_edge_vectors(R, plan, cell).requires_grad_(True)
            with torch.enable_grad():
                E_mol, _, _ = self._energy(R.detach(), plan, V=V, Vint=Vint)
                if Vint is None:
                    G = torch.autograd.grad(E_mol, V, grad_outputs=self._cotangent(E_mol, 0))[0]
                else:
                    G, Gint = torch.autograd.grad(E_mol, (V, Vint), grad_outputs=self._cotangent(E_mol, 0), allow_unused=True)
        if Vint is None:
            return E_mol.detach(), pbc.forces(G, plan), pbc.stress(V.detach(), G, plan, cell)
        G = torch.zeros_like(V) if G is None else G
        Gint = torch.zeros_like(Vint) if Gint is None else Gint
        return E_mol.detach(), pbc.forces_q(G, Gint, plan), pbc.stress_q(V.detach(), G, Vint.detach(), Gint, plan, cell)

    def _forward_periodic_direct(self, R, plan, cell):
        """E, F (A,1,3) of a periodic batch from a direct-force model (`periodic_direct_forces`): nothing is differentiated, so
        the pass runs without autograd and with constant weights (the LDS-resident Dense stacks, the fused aggregation), the
        output blocks' force terms are stacked into one (K,E,1) array and the force head — sum over the blocks, the coupling of
        the two directions of an edge through `plan.id_swap`, the unit vectors, the sum over the in-edges — is one launch
        (pbc.direct_forces, csrc/direct_force.hip)."""
        from .. import pbc
        V = pbc.edge_vectors(R, plan, cell)
        with torch.no_grad(), ops.weight_cache(self._wcache), ops.fused_first_order(True), ops.param_grads(False), \
                ops.train2(False, None), ops.chain_mode(self.matmul_precision), ops.position_graph(False):
            E_mol, terms, _ = self._energy(R.detach(), plan, V=V, force_terms=True)
            F = pbc.direct_forces(torch.stack(terms), V, plan, self.forces_coupled)
        return E_mol, F

    def _forward_periodic_direct_train(self, R, plan, cell):
        """E, F (A,1,3) of a periodic batch from a direct-force model in training mode (`periodic_direct_forces` and
        `periodic_training`), both with an autograd graph to the parameters.  Nothing is differentiated twice: the training
        step of a direct-force model is one first-order backward.  Two forms with parameter gradients:
          * widths the split-operand chain kernel takes (`_train2_widths_ok`; any width on the host emulation), arithmetic not
            "f32": the Dense stacks as single-launch chain programs with trainable weights (ops_train.stack under
            `ops.train2`: its first sweep and first adjoint only, the weight gradients through the grouped queue of the train
            step) — 4 x fewer launches than one GEMM per Dense;
          * other widths, `matmul_precision = "f32"`, GEMNET_TRAIN2=0: the fused single-launch layers of the molecular
            direct-force training branch (`fused_first_order(True)`), one launch per Dense and per weight gradient.
        `force_graph = True` selects the composite closure instead (ATen on V: the A/B reference, as for molecules).  V is a
        constant: positions and cell never join an autograd graph.  The force head is `pbc.direct_forces_train`:
        `_forward_periodic_direct`'s one launch, and one launch of its adjoint in the backward.  Under torch.no_grad() the same
        pass records no graph; the constant-weight inference caches are not consulted."""
        from .. import pbc
        V = pbc.edge_vectors(R, plan, cell)
        mode = self.matmul_precision or K_chain_mode()
        t2 = (not self.force_graph and ops.USE_TRAIN2 and mode != "f32" and (not R.is_cuda or self._train2_widths_ok()))
        with ops.weight_cache(self._wcache), ops.fused_first_order(not self.force_graph and not t2), ops.param_grads(True), \
                ops.train2(t2, self._packs if (t2 and R.is_cuda) else None), ops.chain_mode(self.matmul_precision), \
                ops.position_graph(False):
            E_mol, terms, _ = self._energy(R.detach(), plan, V=V, force_terms=True)
            F = pbc.direct_forces_train(terms, V, plan, self.forces_coupled)
        return E_mol, F

    def _forward_periodic_train(self, R, plan, cell, t2):
        """E, F, S of a periodic batch with an autograd graph to the parameters (`periodic_training`): E under the context of
        the molecular training branch, G = -dE/dV with create_graph=True, and F, S linear in G through ONE differentiable
        Function (pbc.force_stress: its backward is the adjoint kernel of csrc/pbc_train.hip).  V is a private leaf — positions
        and cell never join an autograd graph — so `loss.backward()` reaches the parameters through G alone."""
        from .. import pbc
        V = pbc.edge_vectors(R, plan, cell).requires_grad_(True)
        # GemNet-Q (`periodic_quadruplets_training`): the second private leaf Vint, ONE gradient call for both, and F, S linear in
        # (G, Gint) through pbc.force_stress_q (the adjoint kernel once per edge family)
        Vint = None if self.triplets_only else pbc.int_edge_vectors(R, plan, cell).requires_grad_(True)
        with ops.weight_cache(self._wcache), ops.fused_first_order(False), ops.param_grads(True), \
                ops.train2(t2, self._packs if (t2 and R.is_cuda) else None), ops.chain_mode(self.matmul_precision), \
                ops.position_graph(False), torch.enable_grad():
            E_mol, _, _ = self._energy(R.detach(), plan, V=V, Vint=Vint)
            with ops.param_grads(False):  # only dE/dV (and dE/dVint) is needed here
                if Vint is None:
                    G = torch.autograd.grad(E_mol, V, grad_outputs=self._cotangent(E_mol, 0), create_graph=True)[0]
                else:
                    G, Gint = torch.autograd.grad(E_mol, (V, Vint), grad_outputs=self._cotangent(E_mol, 0), create_graph=True,
                                                  allow_unused=True)
            if Vint is None:
                F, S = pbc.force_stress(G, V.detach(), plan, cell)
            else:
                G = torch.zeros_like(V) if G is None else G
                Gint = torch.zeros_like(Vint) if Gint is None else Gint
                F, S = pbc.force_stress_q(G, V.detach(), Gint, Vint.detach(), plan, cell)
        return E_mol, F, S

    def _cotangent(self, E_mol, target):
        """Constant -1 in column `target` (zeros elsewhere) shaped like E_mol, cached per (shape, device)."""
        key = (tuple(E_mol.shape), E_mol.device, E_mol.dtype, target)
        c = self._cot.get(key) if self._cot is not None else None
        if c is None:
            c = torch.zeros(E_mol.shape, device=E_mol.device, dtype=E_mol.dtype)
            c[:, target] = -1.0
            if E_mol.is_cuda and torch.cuda.is_current_stream_capturing():
                return c      # memory of a capture's private pool must not outlive it in a cache
            # never evicted: a hipGraph captured after this call bakes the address in and reads it at every replay
            # (one (n_molecules, n_targets) tensor per distinct batch size: bytes)
            if self._cot is None:
                self._cot = {}
            self._cot[key] = c
        return c

    def _side_stream(self, device, role="out"):
        """One side stream per calling stream (several molecule shards may run this module concurrently) and role
        ("out": the output blocks; "plan": the adjoint-only index structures of a plan built inside a capture)."""
        if self._side is None:
            self._side = {}
        cur = torch.cuda.current_stream(device)
        key = (device.index, cur.cuda_stream) if role == "out" else (device.index, cur.cuda_stream, role)
        st = self._side.get(key)
        if st is None:
            st = torch.cuda.Stream(device=device)
            # torch hands out streams round-robin from a pool of 32: late in a long-lived process the new "side" stream
            # can BE the calling stream (e.g. the capture stream of torch.cuda.graph).  Everything would still be correct
            # (one stream, serial), but the output blocks would then count as same-stream consumers of the gradient sinks
            # and change the summation order — graph replay and eager run would stop being bit-identical.
            taken = {cur.cuda_stream} | {v.cuda_stream for k, v in self._side.items() if k[:2] == key[:2]}
            for _ in range(4):
                if st.cuda_stream not in taken:
                    break
                st = torch.cuda.Stream(device=device)
            self._side[key] = st
        return st

    def train(self, mode=True):
        if bool(mode) != self.training:
            self._wcache = {}   # weights change while training: derived forms cached for inference are stale afterwards
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._wcache = {}  # .to()/.float()/.cuda() replace the parameters' storage
        self._packs.clear()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._wcache = {}
        self._packs.clear()
        return super().load_state_dict(*args, **kwargs)

    def __deepcopy__(self, memo):
        side, self._side = self._side, None  # HIP stream handles are not copyable
        cache, self._wcache = self._wcache, {}  # keyed by this instance's weight addresses
        packs, self._packs = self._packs, ops.PackRegistry()
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            import copy
            for k, v in self.__dict__.items():
                setattr(new, k, copy.deepcopy(v, memo))
            return new
        finally:
            self._side = side
            self._wcache = cache
            self._packs = packs

    @staticmethod
    def _check_inputs(R):
        if not R.is_cuda:
            raise RuntimeError("gemnet_pytorch_amd.GemNet runs on a HIP device only (no CPU fallback); "
                               "move the model and the batch to 'cuda'.")
        if R.dtype != torch.float32:
            raise TypeError("gemnet_pytorch_amd.GemNet computes in fp32; got R of dtype %s" % R.dtype)

    # ----------------------------------------------------------------------------------- misc
    def predict(self, inputs, stress=False):
        """(E, F) detached on the host, as the reference (gemnet.py:780-784).  Inputs from `md.DeviceMolecule.get()` (the MD
        loop of ase_calculator.py:148-170) carry no index arrays: they are served by the device index builder + one
        replayed hipGraph (md.predict_molecule).  A periodic structure (`DeviceMolecule(..., cell=...)` or a batch with
        `cell`): `stress=True` -> (E, F, S)."""
        from ..md import MoleculeInputs, predict_molecule, predict_periodic
        if isinstance(inputs, MoleculeInputs):
            if stress:
                if inputs.get("cell") is None:
                    raise ValueError("stress=True needs a periodic structure")
                return predict_periodic(self, inputs, stress=True, to_host=True)
            return predict_molecule(self, inputs, to_host=True)
        out = self(inputs, stress=stress)
        return tuple(t.detach().cpu() for t in out)

    def load_weights(self, path):
        self.load_state_dict(torch.load(path))

    def save_weights(self, path):
        torch.save(self.state_dict(), path)

    def tf_variable_names(self):
        """parameter name -> variable of the TensorFlow GemNet checkpoint (the copy list of gemnet.py:633-778 as rules;
        pinned against the reference in tests/golden/tf_names.json): '.' -> '/', Dense `weight` -> `kernel`, the
        ResidualLayer members `dense_mlp.<k>` -> `dense_mlp/layer_with_weights-<k>`, the embedding table without leaf."""
        out = {}
        for name, _ in self.named_parameters():
            parts = name.split(".")
            if name == "atom_emb.embeddings.weight":
                parts = parts[:-1]
            elif parts[-1] == "weight":
                parts[-1] = "kernel"
            parts = [f"layer_with_weights-{q}" if i > 0 and parts[i - 1] == "dense_mlp" else q
                     for i, q in enumerate(parts)]
            out[name] = "/".join(parts) + "/.ATTRIBUTES/VARIABLE_VALUE"
        return out

    def load_tfmodel(self, path):
        """Import the weights of a TensorFlow GemNet checkpoint (gemnet.py:617-778): 2-D kernels are transposed
        (TF Dense is (in, out)), the 3-D bilinear kernels and all other variables copied as they are.  `path` is a TF
        checkpoint prefix (needs `tensorflow`, as in the reference) or a `.npz` holding the same variables under the
        same names (`np.savez(f, **{n: reader.get_tensor(n) for n in names})` on a machine that has TensorFlow).
        Unlike the reference — which raises AttributeError on `out_forces/bias` of its bias-free Dense — direct-force
        models load as well."""
        import numpy as np
        if str(path).endswith(".npz"):
            arrays = np.load(path)
            get = lambda n: arrays[n]   # noqa: E731
        else:
            try:
                import tensorflow as tf
            except ImportError as e:
                raise ImportError(
                    "GemNet.load_tfmodel needs TensorFlow to read a TF checkpoint (as the reference does); without it, "
                    "export the checkpoint's variables to a .npz with the same names and pass that file") from e
            get = tf.train.load_checkpoint(path).get_tensor
        with torch.no_grad():
            for name, p in self.named_parameters():
                tf_name = self.tf_variable_names_cached()[name]
                W = torch.as_tensor(np.asarray(get(tf_name)))
                if tf_name.endswith("kernel/.ATTRIBUTES/VARIABLE_VALUE") and W.dim() == 2:
                    W = W.t()
                if tuple(W.shape) != tuple(p.shape):
                    raise ValueError(f"checkpoint variable {tf_name}: shape {tuple(W.shape)} does not fit "
                                     f"parameter {name} {tuple(p.shape)}")
                p.copy_(W.to(p.dtype))
        self._wcache.clear()

    def tf_variable_names_cached(self):
        names = getattr(self, "_tf_names", None)
        if names is None:
            names = self._tf_names = self.tf_variable_names()
        return names
