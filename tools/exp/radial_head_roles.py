"""Lane mapping of the radial head's adjoint: the library kernel (4 edges x 16 lanes per wave, three functions per lane) against
the experiment of tools/exp/radial_head_roles.hip (64 edges x 8 waves, one basis role per wave), on the bench batch: 200 launches
in one graph, best of three replays, three rounds in one session, and the two results compared bit for bit.
    python tools/exp/radial_head_roles.py [rounds]        (builds tools/exp/bin/libradial_head_roles.so when it is missing)"""
import ctypes
import os
import subprocess
import sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
SRC, LIB = os.path.join(HERE, "radial_head_roles.hip"), os.path.join(HERE, "bin", "libradial_head_roles.so")


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= os.path.getmtime(SRC):
        return
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared",
                           "-fPIC", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", SRC, "-o", LIB])


if __name__ == "__main__":
    build()
    if len(sys.argv) > 1 and sys.argv[1] == "build":
        sys.exit(0)
    import torch
    from gemnet_pytorch_amd import kernels as K
    from gemnet_pytorch_amd.graph import GraphPlan
    from gemnet_pytorch_amd.model.gemnet import GemNet
    from tools.gemm_bench import graph_best
    import bench

    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.exp_radial_head_bwd_roles.argtypes = [vp] * 13 + [ctypes.c_int64, ctypes.c_float, ctypes.c_int, vp]
    cfg = dict(bench.GEMNET_T)
    torch.manual_seed(1234)
    model = GemNet(**cfg, scale_file=bench.SCALE_FILE).to("cuda")
    inputs, _ = bench.make_batch(cfg, 32, 32, 0, "cuda")
    plan = GraphPlan.from_inputs(inputs, True)
    R = inputs["R"].float().contiguous()
    ic, ia = plan.id_c.idx32, plan.id_a.idx32
    E = ic.shape[0]
    b3 = model.cbf_basis3
    freq, z, nrm, cutoff, p = model.rbf_basis.frequencies.detach().float().contiguous(), b3.z_ln.float().contiguous(), \
        b3.n_ln.contiguous(), float(b3.cutoff), int(b3.p)
    wcat = K.radial_head_weights(*[d.weight.detach() for d in (model.mlp_rbf3, model.mlp_rbf_h, model.mlp_rbf_out)],
                                 model.mlp_cbf3.weight.detach())
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    gs = [rn(E, 6), rn(E, 16), rn(E, 16), rn(E, 16), rn(E, 7, 16)]
    ptr = lambda t: None if t is None else vp(t.data_ptr())         # noqa: E731

    def roles(cot):
        W = torch.empty(E, 3, device="cuda")
        rc = lib.exp_radial_head_bwd_roles(*[ptr(t) for t in cot], ptr(R), ptr(ic), ptr(ia), ptr(freq), ptr(z), ptr(nrm), ptr(wcat),
                                           ptr(W), E, cutoff, p, vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        return W

    def library(cot):
        return K.radial_head_bwd(*cot, R, ic, ia, freq, z, nrm, wcat, cutoff, p)

    print(f"E={E}")
    for name, cot in (("all five cotangents", gs), ("the model's four (no g_rbf)", [None] + gs[1:]), ("g_rbf_W1 only", [None] * 4 + gs[4:])):
        a, b = library(cot), roles(cot)
        torch.cuda.synchronize()
        print(f"{name}: bit-equal {torch.equal(a, b)}, max |diff| {float((a - b).abs().max()):.3e} at max |W| {float(a.abs().max()):.3e}")
    cot = [None] + gs[1:]
    for _ in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
        print(f"16-lane mapping (library)      : {graph_best(lambda: library(cot)):7.2f} us (200 launches in one graph, best of 3)")
        print(f"one role per wave (experiment) : {graph_best(lambda: roles(cot)):7.2f} us")
