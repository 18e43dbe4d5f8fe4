"""The reference's smooth-dynamics stages as functions on a caller's ``Data`` (``_src/smooth.py:34-467, 500-521``): ``kinematics``, ``com_pos``, ``crb``,
``tendon_armature``, ``factor_m``, ``com_vel`` and ``rne(m, d, flg_acc=False)``.  Each reads the leaves of ``d`` AS THEY ARE -- nothing is recomputed from ``qpos``, so
a stage can be run again after an edit of the leaves it reads -- and returns ``d.replace(...)`` with exactly its own leaves as fresh tensors; every other leaf of the
result is the caller's tensor object, and nothing is written to the input.

===================  ===========================================================  ==========================================  =====================================
function             reads from ``d``                                             model values                                leaves replaced
===================  ===========================================================  ==========================================  =====================================
``kinematics``       ``qpos``, ``mocap_pos``, ``mocap_quat`` (``subtree_com`` for  --                                          ``qpos`` (quaternions normalised),
                     trackcom / targetbodycom cameras, the caller's)                                                           ``xanchor`` .. ``light_xdir``
``com_pos``          ``xipos``, ``ximat``, ``xmat``, ``xanchor``, ``xaxis``       ``body_mass``, ``body_inertia``             ``subtree_com``, ``cinert``, ``cdof``
``crb``              ``cinert``, ``cdof``                                         ``dof_armature``                            ``crb`` (row 0 zero), ``qM`` (dense)
``tendon_armature``  ``qM``, ``ten_J``                                            the tendons' armature                       ``qM``; ``d`` itself without tendons
``factor_m``         ``qM`` (its lower triangle)                                  --                                          ``qLD`` (``L``, zeros above)
``com_vel``          ``cdof``, ``qvel``                                           --                                          ``cvel``, ``cdof_dot``
``rne``              ``cdof``, ``cdof_dot``, ``cvel``, ``cinert``, ``qvel``,      ``opt.gravity``, ``opt.disableflags``       ``qfrc_bias``
                     ``qacc`` with ``flg_acc``                                    (GRAVITY)
===================  ===========================================================  ==========================================  =====================================

``kinematics`` has the pass's own inputs, so it is ``forward(m, d, stages=MJH_STAGE_KINEMATICS)`` with only the leaves above taken over, bit for bit.  The other six
are one native launch each (``mjh_smooth``, ``csrc/mjh_smooth.h``, whose header states the definitions and the order of every sum); ``factor_m`` is the reference's
``math.small_cholesky``: up to 16 dofs the scalar sequence with every pivot clamped at 1e-12, above ``qM + 1e-10 I``.

The model VALUES are read from the caller's ``Model`` at each call (``tendon_armature``, no ``Model`` field: from the compiled model the tables keep), so a value-only
edit such as ``mx.replace(body_mass=...)`` takes effect without a new native model; the structure (the tree, the joints) is the compiled model's.  A leaf the model
makes empty (``nv == 0``, no tendons, ``B == 0``) yields an empty result and no launch.  A model one environment of which does not fit the LDS of a CU is refused with
a ``RuntimeError`` naming the sizes (``plan``).

Every leading dimension of a leaf is the batch (S); matrices may come as ``(n, 3, 3)`` or ``(n, 9)``.  The calls run on the caller's current stream.  ``torch.vmap`` /
``torch.compile``: there is no operator for these functions; they raise ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import native
from ._postpass import bind, call, check_leaves, model_value, probe, refuse_tracing, require_device

COM_POS, CRB, TENDON_ARMATURE, FACTOR_M, COM_VEL, RNE = range(6)  # include/mjhip.h MJH_SMOOTH_*
OPS = dict(com_pos=COM_POS, crb=CRB, tendon_armature=TENDON_ARMATURE, factor_m=FACTOR_M, com_vel=COM_VEL, rne=RNE)
STAGE_KINEMATICS = 0x001  # include/mjhip.h MJH_STAGE_KINEMATICS
KINEMATICS_LEAVES = ("qpos", "xanchor", "xaxis", "xpos", "xquat", "xmat", "xipos", "ximat", "geom_xpos", "geom_xmat", "site_xpos", "site_xmat", "cam_xpos", "cam_xmat",
                     "light_xpos", "light_xdir")


def _sizes(m):
    return dict(nb=int(m.nbody), nj=int(m.njnt), nv=int(m.nv), nt=int(m.ntendon))


def _tails(m):
    z = _sizes(m)
    nb, nj, nv, nt = z["nb"], z["nj"], z["nv"], z["nt"]
    return dict(xipos=(nb, 3), ximat=(nb, 3, 3), xmat=(nb, 3, 3), xanchor=(nj, 3), xaxis=(nj, 3), cinert=(nb, 10), cdof=(nv, 6), cdof_dot=(nv, 6), cvel=(nb, 6),
                qvel=(nv,), qacc=(nv,), qM=(nv, nv), ten_J=(nt, nv))


def plan(op, nbody: int, nv: int, ntendon: int, dtype) -> tuple[int, int, int]:
    """(lanes per environment, environments per workgroup, reals of LDS per environment) of one call of ``op`` (a function's name or its ``MJH_SMOOTH_*`` number): the
    library's own plan (``mjh_smooth_plan``, a host computation).  A model one environment of which exceeds the LDS of a CU is a ``RuntimeError`` naming the sizes."""
    op = OPS[op] if isinstance(op, str) else int(op)
    lib = native.load_library()
    fn = getattr(lib, "mjh_smooth_plan", None)
    if fn is None:
        raise RuntimeError(f"{native.LIB_PATH} predates the smooth-dynamics functions (no mjh_smooth_plan): rebuild the library")
    out = (ctypes.c_int * 3)()
    real = 8 if dtype == torch.float64 else 4
    rc = fn(op, int(nbody), int(nv), int(ntendon), real, out)
    if rc == -12:
        raise RuntimeError(f"{list(OPS)[op]}: nbody = {nbody}, nv = {nv}, ntendon = {ntendon} in {dtype} need {out[2] * real} bytes of LDS per environment; "
                           f"a CU has {160 * 1024}")
    if rc != 0:
        raise RuntimeError(f"smooth.plan failed ({rc}): {lib.mjh_last_error().decode()}")
    return tuple(out)


def _value(name, m, field, shape, dtype, device):
    v = getattr(m, field) if hasattr(m, field) else getattr(m.tables.source, field)
    got = tuple(np.shape(v))
    if got != shape:
        raise ValueError(f"{name}: Model.{field} has shape {got}, expected {shape}")
    return model_value(m, field, v, dtype, device)


def _run(name, m, leaves: dict, probe_leaf: str, values: dict, outs: dict, **scalars):
    """One ``mjh_smooth`` call: the checks in the order of ``integrate`` (tracing, shapes / dtype / device, the model values, the CPU refusal), then the launch.
    ``outs``: {args field: trailing shape}; returns {args field: tensor}."""
    refuse_tracing(name, *leaves.values())
    tails = _tails(m)
    batch, dtype, device = probe(name, m, probe_leaf, leaves[probe_leaf], tails[probe_leaf])
    check_leaves(name, leaves, tails, batch, dtype, device, 3)
    z = _sizes(m)
    vals = {n: _value(name, m, field, tuple(z[s] if isinstance(s, str) else s for s in shape), dtype, device) for n, (field, shape) in values.items()}
    require_device(device)
    B = int(math.prod(batch)) if batch else 1
    res = {n: torch.empty(batch + tail, dtype=dtype, device=device) for n, tail in outs.items()}
    if B > 0 and any(t.numel() for t in res.values()):
        plan(OPS[name], z["nb"], z["nv"], z["nt"], dtype)
        a = native.SmoothArgs(op=OPS[name], B=B, **scalars)
        bind(a, dict(leaves, **vals, **res))
        call(name, m, "mjh_smooth", a, device, dtype, what="the smooth-dynamics functions")
    return res


def kinematics(m, d):
    """Forward kinematics from ``d.qpos`` (and the mocap leaves): the reference's ``smooth.kinematics``.  Returns ``d`` with ``qpos`` (quaternions normalised), ``xanchor``,
    ``xaxis``, ``xpos``, ``xquat``, ``xmat``, ``xipos``, ``ximat`` and the geom / site / camera / light frames replaced -- the kinematics stage of the pass itself,
    bit for bit; ``subtree_com``, ``cinert`` and ``cdof`` (the pass computes them in the same stage) stay the caller's: that is ``com_pos``."""
    from .forward import forward

    refuse_tracing("kinematics", d.qpos)
    probe("kinematics", m, "qpos", d.qpos, (int(m.nq),))
    f = forward(m, d, stages=STAGE_KINEMATICS)
    return d.replace(**{n: getattr(f, n) for n in KINEMATICS_LEAVES})


def com_pos(m, d):
    """``subtree_com``, ``cinert`` and ``cdof`` from the caller's ``xipos``, ``ximat``, ``xmat``, ``xanchor`` and ``xaxis`` and the Model's ``body_mass`` / ``body_inertia``:
    the reference's ``smooth.com_pos``."""
    z = _sizes(m)
    r = _run("com_pos", m, dict(xipos=d.xipos, ximat=d.ximat, xmat=d.xmat, xanchor=d.xanchor, xaxis=d.xaxis), "xipos",
             dict(body_mass=("body_mass", ("nb",)), body_inertia=("body_inertia", ("nb", 3))),
             dict(subtree_com_out=(z["nb"], 3), cinert_out=(z["nb"], 10), cdof_out=(z["nv"], 6)))
    return d.replace(subtree_com=r["subtree_com_out"], cinert=r["cinert_out"], cdof=r["cdof_out"])


def crb(m, d):
    """The composite inertias ``crb`` (row 0 zero) and the dense, symmetric ``qM`` (``dof_armature`` on its diagonal) from the caller's ``cinert`` and ``cdof``: the
    reference's ``smooth.crb``."""
    z = _sizes(m)
    r = _run("crb", m, dict(cinert=d.cinert, cdof=d.cdof), "cinert", dict(dof_armature=("dof_armature", ("nv",))), dict(crb_out=(z["nb"], 10), qM_out=(z["nv"], z["nv"])))
    return d.replace(crb=r["crb_out"], qM=r["qM_out"])


def tendon_armature(m, d):
    """``qM + ten_J^T diag(tendon_armature) ten_J`` from the caller's ``qM`` and ``ten_J``: the reference's ``smooth.tendon_armature``; ``d`` itself for a model without
    tendons."""
    z = _sizes(m)
    if z["nt"] == 0:
        return d
    r = _run("tendon_armature", m, dict(qM=d.qM, ten_J=d.ten_J), "qM", dict(tendon_armature=("tendon_armature", ("nt",))), dict(qM_out=(z["nv"], z["nv"])))
    return d.replace(qM=r["qM_out"])


def factor_m(m, d):
    """``qLD``: the Cholesky factor ``L`` of the caller's ``qM`` (its lower triangle is read), zeros above the diagonal -- the reference's ``smooth.factor_m`` on the dense
    path, ``math.small_cholesky``."""
    z = _sizes(m)
    r = _run("factor_m", m, dict(qM=d.qM), "qM", {}, dict(qLD_out=(z["nv"], z["nv"])))
    return d.replace(qLD=r["qLD_out"])


def com_vel(m, d):
    """``cvel`` and ``cdof_dot`` from the caller's ``cdof`` and ``qvel``: the reference's ``smooth.com_vel``."""
    z = _sizes(m)
    r = _run("com_vel", m, dict(cdof=d.cdof, qvel=d.qvel), "qvel", {}, dict(cvel_out=(z["nb"], 6), cdof_dot_out=(z["nv"], 6)))
    if z["nv"] == 0:
        r["cvel_out"].zero_()  # (no dofs, no launch: every body is at rest)
    return d.replace(cvel=r["cvel_out"], cdof_dot=r["cdof_dot_out"])


def rne(m, d, flg_acc: bool = False):
    """``qfrc_bias`` by the recursive Newton-Euler algorithm from the caller's ``cdof``, ``cdof_dot``, ``cvel``, ``cinert`` and ``qvel`` (and ``qacc`` with ``flg_acc``),
    under the Model's ``opt.gravity`` and ``DisableBit.GRAVITY``: the reference's ``smooth.rne``."""
    z = _sizes(m)
    leaves = dict(cdof=d.cdof, cdof_dot=d.cdof_dot, cvel=d.cvel, cinert=d.cinert, qvel=d.qvel)
    if flg_acc:
        leaves["qacc"] = d.qacc
    g = m.opt.gravity
    g = [float(x) for x in (g.detach().cpu().reshape(-1).tolist() if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64).reshape(-1))]
    if len(g) != 3:
        raise ValueError(f"rne: Model.opt.gravity has {len(g)} entries, expected 3")
    r = _run("rne", m, leaves, "qvel", {}, dict(qfrc_bias_out=(z["nv"],)), flg_acc=int(bool(flg_acc)), disableflags=int(m.opt.disableflags), gravity_x=g[0],
             gravity_y=g[1], gravity_z=g[2])
    return d.replace(qfrc_bias=r["qfrc_bias_out"])
