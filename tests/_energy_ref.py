"""A plain numpy reference of energy / energy_pos / energy_vel and the joint / tendon limit and energy sensors (csrc/mjh_energy.h), for the tests only.

It evaluates the definitions in longdouble from the leaves of a pass ({name: array [B, ...]}) and the compiled host model, one environment at a time, and returns
with every value A = the sum of the absolute values of the terms it is a sum of and n = their number, so that a test can hold an implementation in a number format
of unit roundoff u to |got - ref| <= 4 n u A: (n - 1) u A bounds a sum of n terms in ANY order, forming a term takes a few more roundings (two or three products,
a subtraction), and the factor 4 covers those, a contracted multiply-add and a two-stage sum.

Terms.  V: per body three, -mass g_i xipos_i; per slide / hinge spring one, 1/2 k (q - q_spring)^2; per free joint three translational ones and, like a ball joint,
three rotational ones 1/2 k phi_i^2; per tendon spring one.  T: the nv^2 terms 1/2 v_r M_rk v_k.  jointlimitpos / tendonlimitpos: the three terms position
(angle), range, margin;
jointlimitvel / tendonlimitvel: the nv terms J_k v_k; jointlimitfrc / tendonlimitfrc: efc_force[row] itself (A = 0: bit for bit)."""
import numpy as np
import torch

HP = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
U = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24, np.dtype("float64"): 2.0 ** -53, np.dtype("float32"): 2.0 ** -24}
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
JLPOS, JLVEL, JLFRC, TLPOS, TLVEL, TLFRC, EPOT, EKIN = 20, 21, 22, 23, 24, 25, 43, 44
TYPES = (JLPOS, JLVEL, JLFRC, TLPOS, TLVEL, TLFRC, EPOT, EKIN)
D_CONSTRAINT, D_LIMIT, D_SPRING, D_DAMPER, D_GRAVITY, D_SENSOR = 1 << 0, 1 << 3, 1 << 5, 1 << 6, 1 << 7, 1 << 13
PI = 4 * np.arctan(HP(1))
LEAVES = ("qpos", "qvel", "xipos", "ten_length", "qM", "efc_J", "efc_force")


def _np(x):
    x = x.data if not isinstance(x, (torch.Tensor, np.ndarray)) and isinstance(getattr(x, "data", None), torch.Tensor) else x  # (an UnbatchedTensor)
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def model_values(mx, dtype=None):
    """The compiled host model as the definitions need it: the values rounded through `dtype` (default: the model's), as every implementation reads them."""
    dtype = dtype or mx.qpos0.dtype
    src = mx.tables.source
    r = lambda v: torch.as_tensor(_np(v).astype(np.float64)).to(dtype).to(torch.float64).numpy().astype(HP)
    get = lambda n: getattr(mx, n) if hasattr(mx, n) else getattr(src, n)
    nt = int(mx.ntendon)
    V = dict(nq=int(mx.nq), nv=int(mx.nv), nbody=int(mx.nbody), njnt=int(mx.njnt), ntendon=nt, flags=int(mx.opt.disableflags), gravity=r(mx.opt.gravity),
             jnt_type=_np(mx.jnt_type).astype(np.int64), jnt_qposadr=_np(mx.jnt_qposadr).astype(np.int64), jnt_limited=_np(mx.jnt_limited).astype(bool))
    for n in ("body_mass", "jnt_stiffness", "qpos_spring", "jnt_range", "jnt_margin"):
        V[n] = r(get(n))
    for n in ("tendon_stiffness", "tendon_lengthspring", "tendon_range", "tendon_margin"):
        V[n] = r(get(n)) if nt else np.zeros((0, 2) if n in ("tendon_lengthspring", "tendon_range") else (0,), dtype=HP)
    V["tendon_limited"] = _np(get("tendon_limited")).astype(bool) if nt else np.zeros(0, dtype=bool)
    V["sizes"] = tuple(int(x) for x in mx.constraint_sizes_py)
    ns = int(getattr(mx, "nsensor", 0) or 0)
    V["sensors"] = [(int(_np(mx.sensor_type)[i]), int(_np(mx.sensor_adr)[i]), int(_np(mx.sensor_objid)[i]), int(_np(src.sensor_datatype)[i]),
                     float(r(np.asarray(mx.sensor_cutoff, dtype=np.float64)[i:i + 1])[0])) for i in range(ns)]
    V["nsensordata"] = int(getattr(mx, "nsensordata", 0) or 0)
    return V


def limit_rows(V):
    """{("jnt", j) | ("tendon", t): the row of its limit in efc_J / efc_force}: equality, frictionloss, ball limits, slide / hinge limits, tendon limits."""
    if V["flags"] & (D_CONSTRAINT | D_LIMIT):
        return {}
    ne, nf = V["sizes"][0], V["sizes"][1]
    lim = [j for j in range(V["njnt"]) if V["jnt_limited"][j]]
    ball = [j for j in lim if V["jnt_type"][j] == BALL]
    sh = [j for j in lim if V["jnt_type"][j] in (SLIDE, HINGE)]
    ten = [t for t in range(V["ntendon"]) if V["tendon_limited"][t]]
    rows = {("jnt", j): ne + nf + i for i, j in enumerate(ball)}
    rows.update({("jnt", j): ne + nf + len(ball) + i for i, j in enumerate(sh)})
    rows.update({("tendon", t): ne + nf + len(ball) + len(sh) + i for i, t in enumerate(ten)})
    return rows


def quat_mul(u, v):
    return np.array([u[0] * v[0] - u[1] * v[1] - u[2] * v[2] - u[3] * v[3], u[0] * v[1] + u[1] * v[0] + u[2] * v[3] - u[3] * v[2],
                     u[0] * v[2] - u[1] * v[3] + u[2] * v[0] + u[3] * v[1], u[0] * v[3] + u[1] * v[2] - u[2] * v[1] + u[3] * v[0]])


def _atan2(y, x):
    return np.arctan2(np.asarray(y, dtype=HP), np.asarray(x, dtype=HP))


def axis_angle(q):
    """(axis, angle in (-pi, pi]) of a quaternion (not necessarily of unit length)."""
    s = np.sqrt((q[1:] ** 2).sum())
    axis = q[1:] / s if s > 0 else np.zeros(3, dtype=q.dtype)
    a = 2 * _atan2(s, q[0])
    if a > PI:
        a = a - 2 * PI
    return axis, a


def rotation_vector(q, qs):
    """phi of quat_spring^-1 o normalize(quat)."""
    u = q / np.sqrt((q ** 2).sum())
    vi = np.array([qs[0], -qs[1], -qs[2], -qs[3]])
    axis, a = axis_angle(quat_mul(vi, u))
    return axis * a


def potential(V, qpos, xipos, ten_length):
    """(V, A, n) of one environment."""
    terms = []
    if not V["flags"] & D_GRAVITY:
        for b in range(1, V["nbody"]):
            terms += [-V["body_mass"][b] * V["gravity"][i] * xipos[b, i] for i in range(3)]
    if not V["flags"] & (D_SPRING | D_DAMPER):
        for j in range(V["njnt"]):
            k, t, qa = V["jnt_stiffness"][j], V["jnt_type"][j], V["jnt_qposadr"][j]
            if k == 0:  # (no spring: no term)
                continue
            if t in (FREE, BALL):
                if t == FREE:
                    terms += [k * (qpos[qa + i] - V["qpos_spring"][qa + i]) ** 2 / 2 for i in range(3)]
                    qa += 3
                phi = rotation_vector(qpos[qa:qa + 4], V["qpos_spring"][qa:qa + 4])
                terms += [k * phi[i] ** 2 / 2 for i in range(3)]
            else:
                terms.append(k * (qpos[qa] - V["qpos_spring"][qa]) ** 2 / 2)
        for t in range(V["ntendon"]):
            if V["tendon_stiffness"][t] == 0:
                continue
            lo, hi = V["tendon_lengthspring"][t]
            disp = ten_length[t] - hi if ten_length[t] > hi else (lo - ten_length[t] if ten_length[t] < lo else HP(0))
            terms.append(V["tendon_stiffness"][t] * disp ** 2 / 2)
    terms = np.array(terms, dtype=HP) if terms else np.zeros(0, dtype=HP)
    return terms.sum(), np.abs(terms).sum(), len(terms)


def kinetic(V, qvel, qM):
    """(T, A, n) of one environment."""
    terms = qvel[:, None] * qM.reshape(V["nv"], V["nv"]) * qvel[None, :] / 2
    return terms.sum(), np.abs(terms).sum(), terms.size


def cutoff(v, datatype, c):
    if c > 0:
        if datatype == 0:
            return min(max(v, -c), c)
        if datatype == 1:
            return min(v, c)
    return v


def limit_pos(V, kind, obj, qpos, ten_length):
    """(dist - margin if dist < margin else 0, A, n) of a joint's or tendon's limit."""
    if kind == "tendon":
        x, (r0, r1), margin = ten_length[obj], V["tendon_range"][obj], V["tendon_margin"][obj]
        dist, mag = min(x - r0, r1 - x), abs(x) + max(abs(r0), abs(r1))
    else:
        qa, (r0, r1), margin = V["jnt_qposadr"][obj], V["jnt_range"][obj], V["jnt_margin"][obj]
        if V["jnt_type"][obj] == BALL:
            _, angle = axis_angle(qpos[qa:qa + 4])
            dist, mag = max(r0, r1) - angle, abs(angle) + max(abs(r0), abs(r1))
        else:
            x = qpos[qa]
            dist, mag = min(x - r0, r1 - x), abs(x) + max(abs(r0), abs(r1))
    return (dist - margin if dist < margin else HP(0)), mag + abs(margin), 3


def leaves_of(d, qpos=None, qvel=None):
    """The leaves the definitions read, off a Data (any device), as float64 / longdouble-exact numpy [B, ...]."""
    out = {n: _np(getattr(d, n)) for n in LEAVES}
    if qpos is not None:
        out["qpos"] = _np(qpos)
    if qvel is not None:
        out["qvel"] = _np(qvel)
    B = int(np.prod(out["qpos"].shape[:-1])) if out["qpos"].ndim > 1 else 1
    return {n: v.reshape((B,) + v.shape[out["qpos"].ndim - 1:]) for n, v in out.items()}


def evaluate(mx, leaves, values=None):
    """{"energy": (val [B, 2], A [B, 2], n [B, 2]), "sensors": [dict(type, adr, value [B], A [B], n)] for the eight types}, in longdouble."""
    V = values or model_values(mx)
    L = {n: np.asarray(v).astype(HP) for n, v in leaves.items()}
    B = L["qpos"].shape[0]
    nv = V["nv"]
    rows = limit_rows(V)
    en = np.zeros((B, 2), dtype=HP); A = np.zeros((B, 2), dtype=HP); N = np.zeros((B, 2), dtype=np.int64)
    sens = [dict(type=t, adr=adr, obj=obj, value=np.zeros(B, dtype=HP), A=np.zeros(B, dtype=HP), n=0, row=-1)
            for (t, adr, obj, dt, cut) in V["sensors"] if t in TYPES and not V["flags"] & D_SENSOR]
    meta = [s for s in V["sensors"] if s[0] in TYPES and not V["flags"] & D_SENSOR]
    for e in range(B):
        ten = L["ten_length"][e] if V["ntendon"] else np.zeros(0, dtype=HP)
        en[e, 0], A[e, 0], N[e, 0] = potential(V, L["qpos"][e], L["xipos"][e].reshape(-1, 3), ten)
        en[e, 1], A[e, 1], N[e, 1] = kinetic(V, L["qvel"][e], L["qM"][e])
        for s, (t, adr, obj, dt, cut) in zip(sens, meta):
            kind = "tendon" if t in (TLPOS, TLVEL, TLFRC) else "jnt"
            row = rows.get((kind, obj), -1) if t not in (EPOT, EKIN) else -1
            s["row"] = row
            if t == EPOT:
                v, a, n = en[e, 0], A[e, 0], N[e, 0]
            elif t == EKIN:
                v, a, n = en[e, 1], A[e, 1], N[e, 1]
            elif row < 0:
                v, a, n = HP(0), HP(0), 0
            elif t in (JLPOS, TLPOS):
                v, a, n = limit_pos(V, kind, obj, L["qpos"][e], ten)
            elif t in (JLVEL, TLVEL):
                terms = L["efc_J"][e].reshape(-1, nv)[row] * L["qvel"][e]
                v, a, n = terms.sum(), np.abs(terms).sum(), nv
            else:
                v, a, n = L["efc_force"][e][row], HP(0), 0
            s["value"][e], s["A"][e], s["n"] = cutoff(v, dt, cut), a, n
    return dict(energy=(en, A, N), sensors=sens)


def bound(n, u, A):
    """4 n u A."""
    return 4.0 * np.asarray(n, dtype=np.float64) * float(u) * np.asarray(A, dtype=np.float64)
