"""The tests' own reference for com_pos / crb / tendon_armature / factor_m / com_vel / rne (mujoco_torch_amd/smooth.py, csrc/mjh_smooth.h): the six definitions restated
in numpy ``longdouble``, per environment, from the leaves each function reads.  Pinned on the reference's recordings by tests/test_smooth_host.py.

Spatial vectors are [rotational(3), translational(3)] about subtree_com[body_rootid[b]]; bodies are in depth-first order, so a subtree is a range of bodies.  The
factorisation rule is taken as the DEFINITION of the matrix that is factored: for nv > 16 it is qM + 1e-10 I, for nv <= 16 qM itself (pivots clamped at 1e-12)."""
import numpy as np

HP = np.longdouble
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
GRAVITY = 1 << 7
MINVAL = 1e-15
INLINE = 16
FUNCTIONS = ("kinematics", "com_pos", "crb", "tendon_armature", "factor_m", "com_vel", "rne")
# what each function reads of a Data and what it replaces
READS = dict(com_pos=("xipos", "ximat", "xmat", "xanchor", "xaxis"), crb=("cinert", "cdof"), tendon_armature=("qM", "ten_J"), factor_m=("qM",),
             com_vel=("cdof", "qvel"), rne=("cdof", "cdof_dot", "cvel", "cinert", "qvel", "qacc"))
WRITES = dict(kinematics=("qpos", "xanchor", "xaxis", "xpos", "xquat", "xmat", "xipos", "ximat", "geom_xpos", "geom_xmat", "site_xpos", "site_xmat", "cam_xpos",
                          "cam_xmat", "light_xpos", "light_xdir"),
              com_pos=("subtree_com", "cinert", "cdof"), crb=("crb", "qM"), tendon_armature=("qM",), factor_m=("qLD",), com_vel=("cvel", "cdof_dot"),
              rne=("qfrc_bias",))
PASS_LEAVES = ("qpos", "qvel", "qacc", "xipos", "ximat", "xmat", "xanchor", "xaxis", "subtree_com", "cinert", "cdof", "crb", "qM", "qLD", "ten_J", "cvel", "cdof_dot",
               "qfrc_bias")


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else (x.data if hasattr(x, "data") and not isinstance(x, np.ndarray) else x))


def model_values(m, **edits):
    """What the six functions read of a Model (the caller's values, the compiled structure), as numpy; ``edits`` override entries."""
    src = m.tables.source
    I = lambda n: _np(getattr(m, n)).astype(np.int64)
    V = dict(nb=int(m.nbody), nv=int(m.nv), nj=int(m.njnt), nt=int(m.ntendon), body_parentid=I("body_parentid"), body_rootid=I("body_rootid"),
             body_jntadr=I("body_jntadr"), body_jntnum=I("body_jntnum"), jnt_type=I("jnt_type"), jnt_dofadr=I("jnt_dofadr"), jnt_bodyid=I("jnt_bodyid"),
             dof_bodyid=I("dof_bodyid"), dof_parentid=I("dof_parentid"), body_mass=_np(m.body_mass).astype(HP), body_inertia=_np(m.body_inertia).astype(HP),
             dof_armature=_np(m.dof_armature).astype(HP), tendon_armature=np.asarray(getattr(src, "tendon_armature", np.zeros(0)), dtype=np.float64).astype(HP),
             gravity=_np(m.opt.gravity).astype(HP).reshape(3), disableflags=int(m.opt.disableflags))
    V.update(edits)
    return V


def shaped(V, n, a, nbatch=0):
    """A recorded or device leaf in its full trailing shape behind ``nbatch`` batch dimensions (matrices may come flattened)."""
    nb, nv, nj, nt = V["nb"], V["nv"], V["nj"], V["nt"]
    tails = dict(xipos=(nb, 3), ximat=(nb, 3, 3), xmat=(nb, 3, 3), xanchor=(nj, 3), xaxis=(nj, 3), subtree_com=(nb, 3), cinert=(nb, 10), crb=(nb, 10), cdof=(nv, 6),
                 cdof_dot=(nv, 6), cvel=(nb, 6), qvel=(nv,), qacc=(nv,), qfrc_bias=(nv,), qM=(nv, nv), qLD=(nv, nv), ten_J=(nt, nv))
    a = np.asarray(a)
    return a.reshape(a.shape[:nbatch] + tails[n]) if n in tails else a


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=HP)


def inert_mul(i, v):
    tri = np.array([[i[0], i[3], i[4]], [i[3], i[1], i[5]], [i[4], i[5], i[2]]], dtype=HP)
    pos, mass = i[6:9], i[9]
    return np.concatenate([tri @ v[:3] + _cross(pos, v[3:]), mass * v[3:] - _cross(pos, v[:3])])


def motion_cross(u, v):
    return np.concatenate([_cross(u[:3], v[:3]), _cross(u[3:], v[:3]) + _cross(u[:3], v[3:])])


def motion_cross_force(v, f):
    return np.concatenate([_cross(v[:3], f[:3]) + _cross(v[3:], f[3:]), _cross(v[:3], f[3:])])


def _subtree(V, x):
    """The sum of x over every body's subtree (children into parents, last body first)."""
    s = np.array(x, dtype=HP)
    for b in range(V["nb"] - 1, 0, -1):
        s[V["body_parentid"][b]] += s[b]
    return s


def _joints(V, b):
    return range(int(V["body_jntadr"][b]), int(V["body_jntadr"][b]) + int(V["body_jntnum"][b])) if V["body_jntnum"][b] > 0 else range(0)


def com_pos(V, L):
    nb = V["nb"]
    xipos, ximat, xmat = (np.asarray(L[n], dtype=HP) for n in ("xipos", "ximat", "xmat"))
    xanchor, xaxis = np.asarray(L["xanchor"], dtype=HP), np.asarray(L["xaxis"], dtype=HP)
    mass = _subtree(V, V["body_mass"])
    pos = _subtree(V, xipos * V["body_mass"][:, None])
    com = np.where((mass < MINVAL)[:, None], xipos, pos / np.maximum(mass, HP(MINVAL))[:, None])
    cinert = np.zeros((nb, 10), dtype=HP)
    for b in range(nb):
        off = xipos[b] - com[V["body_rootid"][b]]
        h = np.stack([_cross(off, -np.eye(3, dtype=HP)[i]) for i in range(3)])
        I = (ximat[b] * V["body_inertia"][b]) @ ximat[b].T + (h @ h.T) * V["body_mass"][b]
        cinert[b] = np.concatenate([[I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]], off * V["body_mass"][b], [V["body_mass"][b]]])
    cdof = np.zeros((V["nv"], 6), dtype=HP)
    for j in range(V["nj"]):
        t, b, da = int(V["jnt_type"][j]), int(V["jnt_bodyid"][j]), int(V["jnt_dofadr"][j])
        off = com[V["body_rootid"][b]] - xanchor[j]
        if t == FREE:
            cdof[da:da + 3, 3:] = np.eye(3, dtype=HP)
            da += 3
        if t in (FREE, BALL):
            for r in range(3):
                a = xmat[b][:, r]
                cdof[da + r] = np.concatenate([a, _cross(a, off)])
        elif t == HINGE:
            cdof[da] = np.concatenate([xaxis[j], _cross(xaxis[j], off)])
        else:
            cdof[da, 3:] = xaxis[j]
    return dict(subtree_com=com, cinert=cinert, cdof=cdof)


def crb(V, L):
    nv = V["nv"]
    cinert, cdof = np.asarray(L["cinert"], dtype=HP), np.asarray(L["cdof"], dtype=HP)
    c = _subtree(V, cinert)
    c[0] = 0
    qM = np.zeros((nv, nv), dtype=HP)
    for i in range(nv):
        f = inert_mul(c[V["dof_bodyid"][i]], cdof[i])
        j = i
        while j >= 0:
            qM[i, j] = qM[j, i] = f @ cdof[j]
            j = int(V["dof_parentid"][j])
        qM[i, i] += V["dof_armature"][i]
    return dict(crb=c, qM=qM)


def tendon_armature(V, L):
    J = np.asarray(L["ten_J"], dtype=HP)
    return dict(qM=np.asarray(L["qM"], dtype=HP) + J.T @ (J * V["tendon_armature"][:, None]))


def factored_matrix(V, qM):
    """The matrix whose factor qLD is: the lower triangle of qM mirrored, + 1e-10 I above 16 dofs."""
    A = np.tril(np.asarray(qM, dtype=HP))
    A = A + np.tril(A, -1).T
    return A + (HP(1e-10) * np.eye(V["nv"], dtype=HP) if V["nv"] > INLINE else 0)


def factor_m(V, L):
    nv = V["nv"]
    A = factored_matrix(V, L["qM"])
    Lo = np.zeros((nv, nv), dtype=HP)
    for j in range(nv):
        s = A[j, j] - Lo[j, :j] @ Lo[j, :j]
        if nv <= INLINE:
            s = max(s, HP(1e-12))
        Lo[j, j] = np.sqrt(s)
        for r in range(j + 1, nv):
            Lo[r, j] = (A[r, j] - Lo[r, :j] @ Lo[j, :j]) / Lo[j, j]
    return dict(qLD=Lo)


def com_vel(V, L):
    nb, nv = V["nb"], V["nv"]
    cdof, qvel = np.asarray(L["cdof"], dtype=HP), np.asarray(L["qvel"], dtype=HP)
    cvel, dot = np.zeros((nb, 6), dtype=HP), np.zeros((nv, 6), dtype=HP)
    for b in range(1, nb):
        cv = cvel[V["body_parentid"][b]].copy()
        for j in _joints(V, b):
            t, da = int(V["jnt_type"][j]), int(V["jnt_dofadr"][j])
            if t == FREE:
                cv = cv + (cdof[da:da + 3] * qvel[da:da + 3, None]).sum(0)
                da += 3
            w = 1 if t in (HINGE, SLIDE) else 3
            for r in range(w):
                dot[da + r] = motion_cross(cv, cdof[da + r])
            cv = cv + (cdof[da:da + w] * qvel[da:da + w, None]).sum(0)
        cvel[b] = cv
    return dict(cvel=cvel, cdof_dot=dot)


def rne(V, L, flg_acc=False):
    nb, nv = V["nb"], V["nv"]
    cdof, dot, cvel, cinert, qvel = (np.asarray(L[n], dtype=HP) for n in ("cdof", "cdof_dot", "cvel", "cinert", "qvel"))
    cacc = np.zeros((nb, 6), dtype=HP)
    if not V["disableflags"] & GRAVITY:
        cacc[0, 3:] = -V["gravity"]
    own = np.zeros((nb, 6), dtype=HP)
    for i in range(nv):
        own[V["dof_bodyid"][i]] += dot[i] * qvel[i]
        if flg_acc:
            own[V["dof_bodyid"][i]] += cdof[i] * HP(L["qacc"][i])
    loc = np.zeros((nb, 6), dtype=HP)
    for b in range(nb):
        if b > 0:
            cacc[b] = cacc[V["body_parentid"][b]] + own[b]
        loc[b] = inert_mul(cinert[b], cacc[b]) + motion_cross_force(cvel[b], inert_mul(cinert[b], cvel[b]))
    cfrc = _subtree(V, loc)
    return dict(qfrc_bias=np.array([cdof[i] @ cfrc[V["dof_bodyid"][i]] for i in range(nv)], dtype=HP).reshape(nv))


FN = dict(com_pos=com_pos, crb=crb, tendon_armature=tendon_armature, factor_m=factor_m, com_vel=com_vel, rne=rne)


def factor_bound(V, A, u):
    """Backward-error bound of a Cholesky factor computed in precision u: |L L^T - A| <= (n + 1) u / (1 - (n + 1) u) |L| |L|^T entrywise (Higham, Accuracy and
    Stability, thm 10.3), taken as its largest entry, plus the 1e-12 a clamped pivot may add."""
    n = V["nv"]
    g = (n + 1) * u / (1 - (n + 1) * u)
    return g, 1e-12 if n <= INLINE else 0.0


# ---- the recordings (tests/golden/smooth/*.npz, tools/gen_smooth_golden.py) ---------------------------------------------------------------------

import json  # noqa: E402
import os  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smooth")
CASES = ("pendula_f64", "pendula_f32", "ant_f64", "humanoid_f64", "humanoid_f32", "tendon_armature_f64", "centipede_f64", "ant_zero_mass_f64")
KIN_IN = ("qpos", "mocap_pos", "mocap_quat")
_CASES = {}


def tags(V):
    """The recorded runs of a model: the six functions and rne with flg_acc (tendon_armature only with tendons)."""
    return tuple(t for t in ("com_pos", "crb", "tendon_armature", "factor_m", "com_vel", "rne", "rne_acc") if t != "tendon_armature" or V["nt"] > 0)


class Case:
    """One recording: the model (CPU; body_mass edited where the case says so), its values, per environment the pass, the edited inputs and the reference's outputs."""

    def __init__(self, name):
        import torch

        from _util import load_model

        z = np.load(os.path.join(GOLD, name + ".npz"))
        self.name, self.meta = name, json.loads(str(z["meta"]))
        self.dtype = getattr(torch, self.meta["dtype"])
        self.compiled = self.model = load_model(self.meta["xml"], self.meta["overrides"], self.dtype, keep_sensors=self.meta["keep_sensors"])
        if self.meta["zero_mass"]:  # a value-only edit of the caller's Model: the native model keeps the XML's masses
            mass = self.model.body_mass.clone()
            mass[self.meta["zero_mass"]["body"]] = self.meta["zero_mass"]["value"]
            self.model = self.model.replace(body_mass=mass)
        self.V = model_values(self.model)
        self.nenv = self.meta["nenv"]
        self.distance = self.meta["ref_distance"]
        self.kin = [{n: z[f"kin/{e}/{n}"] for n in KIN_IN} for e in range(self.nenv)]
        self.passes = [{n: z[f"pass/{e}/{n}"] for n in PASS_LEAVES} for e in range(self.nenv)]
        self.ins = [{f: {n: z[f"in/{e}/{f}/{n}"] for n in READS[f]} for f in tags(self.V) if f != "rne_acc"} for e in range(self.nenv)]
        self.outs = [{f: {n: z[f"out/{e}/{f}/{n}"] for n in WRITES[f.replace("_acc", "")]} for f in tags(self.V) + ("kinematics",)} for e in range(self.nenv)]

    def data(self, B, device="cpu", fn=None):
        """A Data of B environments, environment i holding recording i % nenv: the recorded pass's leaves, with ``fn``'s edited inputs in place of the pass's
        (``fn='kinematics'``: its recorded inputs)."""
        import torch

        import mujoco_torch_amd as mt

        d = mt.make_data(self.model)
        d = (d if self.dtype == torch.float64 else d.to(self.dtype)).expand(B).clone()
        src = [dict(self.passes[i % self.nenv], **(self.kin[i % self.nenv] if fn == "kinematics" else self.ins[i % self.nenv][fn] if fn else {})) for i in range(B)]
        kw = {n: torch.from_numpy(np.stack([s[n] for s in src]).reshape((B,) + tuple(getattr(d, n).shape[1:]))) for n in src[0]}
        return d.replace(**kw).to(device)


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]
