"""The skinning rule of DESIGN.md 4.17 as a torch statement, with the forward contract around it, a stand-in body module and the
seeded cases of the SMPL tests (tests/test_smpl.py, tests/test_gpu_smpl.py, tools/make_smpl_golden.py).

``lbs`` is written from the definition in the order the reference takes: the joint regressor on the shaped vertices, the pose
features through one matrix product, the kinematic chain as a loop over the joints, a dense weight product.  Run in float64 on
the CPU it is the reference statement (tests/test_smpl.py pins it to the reference's own ``lbs`` to 1e-12); run in float32 it is
the yardstick the device's tolerances are taken from.  Nothing here reads the reference tree or needs a device."""
import numpy as np
import torch

# SMPL's kinematic tree (kintree_table[0] with the root set to -1)
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)

# name -> (V, J, NB, weights per vertex; 0 = dense), in the order of the issue's table
CASES = {
    "single": (4, 1, 1, 1),          # no pose features, no chain
    "chain3": (5, 3, 1, 2),          # the shortest real chain, V below one wave
    "tree": (257, 24, 10, 4),        # SMPL's parent table, V = 4 * 64 + 1
    "wide": (300, 55, 20, 0),        # an SMPL-X-sized skeleton, dense weights: K = J
    "body": (6890, 24, 10, 4),       # SMPL's size: several workgroups of partials
}
# (case, B, identity pose) of every run the bars are measured over and the device is compared on
RUNS = [(n, 1, False) for n in CASES] + [("tree", 2, False), ("tree", 3, False), ("tree", 1, True)]
LOSSES = ("verts", "joints", "both")
OUTPUTS = ("verts", "joints", "grad_betas", "grad_rot")
BUFFERS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")

_cases = {}


def case(name):
    """the model arrays of a case (float32 / int64 numpy, the layouts of the SMPL module's buffers), seeded by the case's position"""
    if name in _cases:
        return _cases[name]
    V, J, NB, per = CASES[name]
    rs = np.random.RandomState(1000 + list(CASES).index(name))
    if J == len(SMPL_PARENTS):
        parents = np.array(SMPL_PARENTS, dtype=np.int64)
    else:
        parents = np.array([-1] + [rs.randint(0, j) if name == "wide" else j - 1 for j in range(1, J)], dtype=np.int64)
    v_template = rs.uniform(-1.0, 1.0, (V, 3))
    shapedirs = 0.03 * rs.randn(V, 3, NB)
    posedirs = 0.01 * rs.randn(9 * (J - 1), 3 * V)
    J_regressor = np.zeros((J, V))
    for j in range(J):                                                     # a few vertices per joint, weights summing to 1
        pick = rs.choice(V, size=min(V, 8), replace=False)
        w = rs.uniform(0.1, 1.0, len(pick))
        J_regressor[j, pick] = w / w.sum()
    lbs_weights = np.zeros((V, J))
    for v in range(V):
        pick = np.arange(J) if per == 0 else rs.choice(J, size=min(per, J), replace=False)
        w = rs.uniform(0.1, 1.0, len(pick))
        lbs_weights[v, pick] = w / w.sum()
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    _cases[name] = dict(v_template=f32(v_template), shapedirs=f32(shapedirs), posedirs=f32(posedirs), J_regressor=f32(J_regressor),
                        parents=parents, lbs_weights=f32(lbs_weights))
    return _cases[name]


def model(name, dtype=torch.float64):
    """the case's arrays as CPU tensors of ``dtype`` (parents int64)"""
    return {k: torch.from_numpy(a) if k == "parents" else torch.from_numpy(a).to(dtype) for k, a in case(name).items()}


def rodrigues(rot_vecs):
    """axis-angle [N,3] -> [N,3,3]: angle = |r + 1e-8|, k = r / angle, I + sin(angle) [k]x + (1 - cos(angle)) [k]x^2"""
    angle = (rot_vecs + 1e-8).norm(dim=1, keepdim=True)
    k = rot_vecs / angle
    z = torch.zeros_like(angle)
    Kx = torch.cat([z, -k[:, 2:3], k[:, 1:2], k[:, 2:3], z, -k[:, 0:1], -k[:, 1:2], k[:, 0:1], z], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device).unsqueeze(0)
    return eye + angle.sin().unsqueeze(1) * Kx + (1 - angle.cos().unsqueeze(1)) * (Kx @ Kx)


def inputs(name, B=1, seed=0, identity=False):
    """(betas [B,NB], rot_mats [B,J,3,3], cotangent on verts [B,V,3], cotangent on joints [B,J,3]), float32 numpy: rotations from
    axis-angles of scale 0.4 plus a perturbation of 0.05 that makes them non-orthonormal (``identity``: the identity, f = 0)"""
    V, J, NB, _ = CASES[name]
    rs = np.random.RandomState(7919 * seed + 31 * list(CASES).index(name) + B)
    betas = rs.randn(B, NB)
    aa = 0.4 * rs.randn(B * J, 3)
    rot = rodrigues(torch.from_numpy(aa)).numpy().reshape(B, J, 3, 3) + 0.05 * rs.randn(B, J, 3, 3)
    if identity:
        rot = np.broadcast_to(np.eye(3), (B, J, 3, 3))
    gv, gj = rs.randn(B, V, 3), rs.randn(B, J, 3)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (betas, rot, gv, gj))


def lbs(betas, rot_mats, m):
    """betas [B,NB], rot_mats [B,J,3,3], m: the six buffers as tensors of one dtype -> verts [B,V,3], joints [B,J,3]"""
    B, Jn = rot_mats.shape[0], rot_mats.shape[1]
    parents = m["parents"].tolist()
    v_shaped = m["v_template"] + torch.einsum("bl,vcl->bvc", betas, m["shapedirs"])
    J = torch.einsum("jv,bvc->bjc", m["J_regressor"], v_shaped)
    feature = (rot_mats[:, 1:] - torch.eye(3, dtype=rot_mats.dtype, device=rot_mats.device)).reshape(B, -1)
    v_posed = v_shaped + (feature @ m["posedirs"]).view(B, -1, 3)
    GR, Gt = [rot_mats[:, 0]], [J[:, 0]]                                   # G_j = G_parent o [R_j | rel_j], as 3x3 and 3
    for j in range(1, Jn):
        p = parents[j]
        rel = J[:, j] - J[:, p]
        GR.append(GR[p] @ rot_mats[:, j])
        Gt.append((GR[p] @ rel.unsqueeze(-1)).squeeze(-1) + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt - (GR @ J.unsqueeze(-1)).squeeze(-1)
    A = torch.cat([GR, At.unsqueeze(-1)], dim=-1)                          # [B,J,3,4]
    T = (m["lbs_weights"] @ A.reshape(B, Jn, 12)).view(B, -1, 3, 4)
    verts = (T[..., :3] @ v_posed.unsqueeze(-1)).squeeze(-1) + T[..., 3]
    return verts, Gt


def run(name, B=1, dtype=torch.float64, seed=0, identity=False):
    """-> {loss: {verts, joints, grad_betas, grad_rot}} (numpy of ``dtype``) for the three losses: the cotangent on verts only, on
    joints only, on both"""
    m = model(name, dtype)
    betas, rot, gv, gj = (torch.from_numpy(a).to(dtype) for a in inputs(name, B, seed, identity))
    out = {}
    for loss in LOSSES:
        b, r = betas.clone().requires_grad_(True), rot.clone().requires_grad_(True)
        verts, joints = lbs(b, r, m)
        total = ((verts * gv).sum() if loss != "joints" else 0) + ((joints * gj).sum() if loss != "verts" else 0)
        gb, gr = torch.autograd.grad(total, (b, r), allow_unused=True)
        gb, gr = (torch.zeros_like(x) if g is None else g for g, x in ((gb, b), (gr, r)))     # J = 1: the joints do not depend on R
        out[loss] = dict(verts=verts.detach().numpy(), joints=joints.detach().numpy(), grad_betas=gb.numpy(), grad_rot=gr.numpy())
    return out


def gap(a, b):
    """||a - b||inf / ||b||inf; where b is all zeros: 0 if a is too, else inf"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    num, den = (np.abs(a - b).max(), np.abs(b).max()) if b.size else (0.0, 0.0)
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return float(num / den)


def measure_gaps(seeds=range(5)):
    """output -> (largest gap of the float32 run against the float64 run over RUNS, the three losses and ``seeds``, where)"""
    torch.set_num_threads(1)                                               # one summation order on every host
    worst = {k: (0.0, None) for k in OUTPUTS}
    for name, B, identity in RUNS:
        for seed in seeds:
            r64, r32 = run(name, B, torch.float64, seed, identity), run(name, B, torch.float32, seed, identity)
            for loss in LOSSES:
                for k in OUTPUTS:
                    g = gap(r32[loss][k], r64[loss][k])
                    if g > worst[k][0]:
                        worst[k] = (g, (name, B, "identity" if identity else "posed", seed, loss))
    return worst


class Selector(torch.nn.Module):
    """an index-select ``vertex_joint_selector``: the joints, then the listed vertices"""

    def __init__(self, idx):
        super().__init__()
        self.register_buffer("extra_joints_idxs", torch.as_tensor(idx, dtype=torch.long))

    def forward(self, vertices, joints):
        return torch.cat([joints, torch.index_select(vertices, 1, self.extra_joints_idxs)], dim=1)


class Output(dict):
    """fields by ``[...]`` and as attributes"""
    __getattr__ = dict.__getitem__


def module_forward(module, betas=None, body_pose=None, global_orient=None, transl=None, return_verts=True, return_full_pose=False,
                   pose2rot=True):
    """the forward contract of an SMPL module around ``lbs``: defaults from the module's parameters, betas expanded to the batch,
    axis-angle through ``rodrigues`` when ``pose2rot``, joints through the module's selector and mapper, transl added to both"""
    global_orient = module.global_orient if global_orient is None else global_orient
    body_pose = module.body_pose if body_pose is None else body_pose
    betas = module.betas if betas is None else betas
    if transl is None and hasattr(module, "transl"):
        transl = module.transl
    full_pose = torch.cat([global_orient, body_pose], dim=1)
    B = max(betas.shape[0], global_orient.shape[0], body_pose.shape[0])
    if betas.shape[0] != B:
        betas = betas.expand(B // betas.shape[0], -1)
    rot = (rodrigues(full_pose.reshape(-1, 3)) if pose2rot else full_pose).reshape(B, -1, 3, 3)
    verts, joints = lbs(betas, rot, {k: getattr(module, k) for k in BUFFERS})
    joints = module.vertex_joint_selector(verts, joints)
    if module.joint_mapper is not None:
        joints = module.joint_mapper(joints)
    if transl is not None:
        joints, verts = joints + transl.unsqueeze(1), verts + transl.unsqueeze(1)
    return Output(vertices=verts if return_verts else None, joints=joints, full_pose=full_pose if return_full_pose else None,
                  global_orient=global_orient, transl=None, betas=betas, body_pose=body_pose)


class StandIn(torch.nn.Module):
    """a body module with the six buffers of a case, the parameters of ``SMPL`` (zeros) and an index-select joint selector; its own
    forward is ``module_forward``"""

    def __init__(self, name, batch_size=1, extra=(0, 3), create_transl=False, dtype=torch.float32):
        super().__init__()
        for k, t in model(name, dtype).items():
            self.register_buffer(k, t)
        V, J, NB, _ = CASES[name]
        self.betas = torch.nn.Parameter(torch.zeros(batch_size, NB, dtype=dtype))
        self.global_orient = torch.nn.Parameter(torch.zeros(batch_size, 3, dtype=dtype))
        self.body_pose = torch.nn.Parameter(torch.zeros(batch_size, 3 * (J - 1), dtype=dtype))
        if create_transl:
            self.transl = torch.nn.Parameter(torch.zeros(batch_size, 3, dtype=dtype))
        self.joint_mapper = None
        self.vertex_joint_selector = Selector(extra)

    def forward(self, **kwargs):
        return module_forward(self, **kwargs)
