"""ctypes binding of the C ABI declared in ``include/mjhip.h``.

PyTorch is used only for device memory and streams; the step itself is the hand-written HIP
library ``libmjhip.so`` (built in-tree by ``__graft_entry__.build()``).  There is NO CPU or
PyTorch fallback: if the library is missing, or the tensors are not on a HIP device, the call
raises.  The structure layouts are derived from the header's X-macro lists so the binding cannot
drift from the ABI.
"""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import torch

from .container import UnbatchedTensor

from .io import model_float_leaves
from .device import static_contact_fields

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_PKG_DIR))
HEADER = os.path.join(_ROOT, "include", "mjhip.h")
LIB_PATH = os.environ.get("MJH_LIB") or os.path.join(os.path.dirname(_PKG_DIR), "lib", "libmjhip.so")  # MJH_LIB: A/B builds

MJH_F64, MJH_F32 = 0, 1
FLAG_FIXED_ITERATIONS = 1
FLAG_INV_DISCRETE = 2  # mjh_inverse: discrete_acc (opt.enableflags & INVDISCRETE)
STAGE_ALL = 0x7F


def _macro_names(text: str, macro: str):
    m = re.search(r"#define\s+" + macro + r"\(X\)(.*?)(?:\n\s*\n|\n#|\ntypedef)", text, re.S)
    if m is None:
        raise RuntimeError(f"{macro} not found in {HEADER}")
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"X\((\w+)\)", body)


def _load_lists():
    with open(HEADER) as f:
        text = f.read()
    return {k: _macro_names(text, k) for k in (
        "MJH_MODEL_INTS", "MJH_MODEL_REALS", "MJH_MODEL_INT_ARRAYS", "MJH_MODEL_REAL_ARRAYS",
        "MJH_DATA_REALS", "MJH_DATA_I32", "MJH_DATA_I64", "MJH_DATA_EXTRA_IN")}


LISTS = _load_lists()
with open(HEADER) as _f:
    ABI_VERSION = int(re.search(r"#define MJH_ABI_VERSION (\d+)", _f.read()).group(1))  # the header is the single source of the version


def _make_structs():
    f = [("abi_version", ctypes.c_int32)]
    f += [(n, ctypes.c_int32) for n in LISTS["MJH_MODEL_INTS"]]
    f += [(n, ctypes.c_double) for n in LISTS["MJH_MODEL_REALS"]]
    f += [(n, ctypes.c_void_p) for n in LISTS["MJH_MODEL_INT_ARRAYS"]]
    f += [(n, ctypes.c_void_p) for n in LISTS["MJH_MODEL_REAL_ARRAYS"]]
    f += [("len_" + n, ctypes.c_int64) for n in LISTS["MJH_MODEL_INT_ARRAYS"] + LISTS["MJH_MODEL_REAL_ARRAYS"]]

    class ModelDesc(ctypes.Structure):
        _fields_ = f

    d = [(n, ctypes.c_void_p) for n in LISTS["MJH_DATA_REALS"] + LISTS["MJH_DATA_I32"] + LISTS["MJH_DATA_I64"] + LISTS["MJH_DATA_EXTRA_IN"]]  # (the trailing input-only leaves: NULL unless a sensor reads them)

    class DataPtrs(ctypes.Structure):
        _fields_ = d

    return ModelDesc, DataPtrs


ModelDesc, DataPtrs = _make_structs()

# Data leaf name -> attribute path on the Data container
DATA_PATH = {n: (("contact", n[len("contact_"):]) if n.startswith("contact_") else (n,)) for n in
             LISTS["MJH_DATA_REALS"] + LISTS["MJH_DATA_I32"] + LISTS["MJH_DATA_I64"]}
DATA_PATH["contact_dim"] = ("contact", "contact_dim")


def _tendon_reals(src, T, dtype):
    """Tendon parameters from the source model, rounded through the compute dtype like every other real table."""
    nt = len(T.tendon["adr"]) - 1
    r = lambda a, shape: np.ascontiguousarray(torch.tensor(np.asarray(a, dtype=np.float64).reshape(shape)).to(dtype).to(torch.float64).numpy()).reshape(-1)
    g = lambda name, shape: r(getattr(src, name), shape) if nt else np.zeros(0)
    return dict(ten_coef=r(T.tendon["coef"], (-1,)), tendon_range=g("tendon_range", (nt, 2)), tendon_margin=g("tendon_margin", (nt,)),
                tendon_invweight0=g("tendon_invweight0", (nt,)), tendon_solref_lim=g("tendon_solref_lim", (nt, 2)),
                tendon_solimp_lim=g("tendon_solimp_lim", (nt, 5)), tendon_stiffness=g("tendon_stiffness", (nt,)),
                tendon_damping=g("tendon_damping", (nt,)), tendon_frictionloss=g("tendon_frictionloss", (nt,)), tendon_solref_fri=g("tendon_solref_fri", (nt, 2)), tendon_solimp_fri=g("tendon_solimp_fri", (nt, 5)), tendon_lengthspring=g("tendon_lengthspring", (nt, 2)), tendon_armature=g("tendon_armature", (nt,)))


def pack_model(m, dtype: torch.dtype):
    """Model -> (ModelDesc, keepalive list of numpy arrays). Floats are evaluated in ``dtype``."""
    T = m.tables
    src = T.source
    ne, nf, nl, ncon, nefc = m.constraint_sizes_py
    ints = dict(
        nq=m.nq, nv=m.nv, nu=m.nu, na=m.na, nbody=m.nbody, njnt=m.njnt, ngeom=m.ngeom, nsite=m.nsite,
        ncam=m.ncam, nlight=m.nlight, nmocap=m.nmocap, ne=ne, nf=len(T.fric_dof), nft=len(T.fric_tendon), nl=len(T.lim_jnt), nlb=len(T.lim_ball_jnt), nlt=int(T.nlt), ncon=ncon, ncand=len(T.con_dim), topk=int(T.topk), nefc=nefc, neq=int(m.neq), neqtab=len(T.eq['kind']), ntendon=int(m.ntendon), nwrapj=len(T.tendon['dof']),
        npair=len(T.pairs), nconvex=0, nsensor=len(T.sensors["type"]), nsensordata=int(getattr(m, "nsensordata", 0) or 0), integrator=int(m.opt.integrator), solver=int(m.opt.solver),
        cone=int(m.opt.cone), disableflags=int(m.opt.disableflags), iterations=int(m.opt.iterations),
        ls_iterations=int(m.opt.ls_iterations),
    )
    f64 = lambda t: np.ascontiguousarray(t.detach().to("cpu", dtype).to(torch.float64).numpy()).reshape(-1)
    grav = f64(m.opt.gravity)
    reals = dict(
        timestep=float(f64(m.opt.timestep)[0]), impratio=float(f64(m.opt.impratio)[0]),
        tolerance=float(m.opt.tolerance), ls_tolerance=float(m.opt.ls_tolerance),
        meaninertia=float(m.stat.meaninertia), gravity_x=float(grav[0]), gravity_y=float(grav[1]), gravity_z=float(grav[2]),
        density=float(f64(m.opt.density)[0]), viscosity=float(f64(m.opt.viscosity)[0]),
        wind_x=float(f64(m.opt.wind)[0]), wind_y=float(f64(m.opt.wind)[1]), wind_z=float(f64(m.opt.wind)[2]),
        magnetic_x=float(f64(m.opt.magnetic)[0]), magnetic_y=float(f64(m.opt.magnetic)[1]), magnetic_z=float(f64(m.opt.magnetic)[2]),
    )
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32)).reshape(-1)
    nu = m.nu
    info = m.actuator_info
    A = lambda name: np.asarray(getattr(m, name))
    int_arrays = dict(
        body_parentid=i32(A("body_parentid")), body_rootid=i32(A("body_rootid")), body_jntadr=i32(A("body_jntadr")),
        body_jntnum=i32(A("body_jntnum")), body_dofadr=i32(A("body_dofadr")), body_dofnum=i32(A("body_dofnum")),
        body_mocapid=i32(A("body_mocapid")), jnt_type=i32(m.jnt_type.data.cpu().numpy()), jnt_qposadr=i32(A("jnt_qposadr")),
        jnt_dofadr=i32(A("jnt_dofadr")), jnt_bodyid=i32(A("jnt_bodyid")), jnt_actfrclimited=i32(A("jnt_actfrclimited")), jnt_actgravcomp=i32(A("jnt_actgravcomp")),
        dof_bodyid=i32(A("dof_bodyid")), dof_jntid=i32(A("dof_jntid")), dof_parentid=i32(A("dof_parentid")),
        geom_type=i32(A("geom_type")), geom_bodyid=i32(A("geom_bodyid")), geom_convexid=-np.ones(m.ngeom, dtype=np.int32),
        site_bodyid=i32(A("site_bodyid")), cam_bodyid=i32(A("cam_bodyid")), cam_mode=i32(A("cam_mode")),
        cam_targetbodyid=i32(A("cam_targetbodyid")), light_bodyid=i32(A("light_bodyid")),
        act_trntype=i32([x[0] for x in info]), act_jnttype=i32([x[2] for x in info]), act_dofadr=i32([x[3] for x in info]),
        act_qposadr=i32([x[4] for x in info]), act_gaintype=i32(m.actuator_gaintype.data.cpu().numpy()),
        act_biastype=i32(m.actuator_biastype.data.cpu().numpy()), act_dyntype=i32(m.actuator_dyntype.data.cpu().numpy()),
        act_ctrllimited=i32(A("actuator_ctrllimited")), act_forcelimited=i32(A("actuator_forcelimited")),
        act_actlimited=i32(A("actuator_actlimited")), act_actadr=i32(A("actuator_actadr")), act_actnum=i32(A("actuator_actnum")),
        sns_type=i32(T.sensors["type"]), sns_adr=i32(T.sensors["adr"]), sns_objid=i32(T.sensors["objid"]), sns_bodyid=i32(T.sensors["bodyid"]),
        sns_rootid=i32(T.sensors["rootid"]), sns_objtype=i32(T.sensors["objtype"]), sns_reftype=i32(T.sensors["reftype"]), sns_refid=i32(T.sensors["refid"]),
        sns_refbodyid=i32(T.sensors["refbodyid"]), sns_refrootid=i32(T.sensors["refrootid"]), sns_datatype=i32(T.sensors["datatype"]), sns_rfadr=i32(T.sensors["rfadr"]),
        rf_geom=i32(T.sensors["rf_geom"]), slot_sensor=i32(T.sensors["slot"]),
        eq_kind=i32(T.eq['kind']), eq_id=i32(T.eq['id']), eq_obj1=i32(T.eq['obj1']), eq_obj2=i32(T.eq['obj2']), eq_row=i32(T.eq['row']), eq_jadr=i32(T.eq['jadr']),
        topk_slot=i32(T.topk_slot), fric_dof=i32(T.fric_dof), fric_tendon=i32(T.fric_tendon), ten_adr=i32(T.tendon['adr']), ten_dof=i32(T.tendon['dof']), ten_qposadr=i32(T.tendon['qpos']), lim_tendon=i32(T.tendon['lim']), act_trnid=i32([x[1] for x in info]),
        lim_ball_jnt=i32(T.lim_ball_jnt), lim_jnt=i32(T.lim_jnt), pair_fn=i32([p[0] for p in T.pairs]), pair_geom1=i32([p[2].geom1 for p in T.pairs]),
        pair_geom2=i32([p[2].geom2 for p in T.pairs]), pair_ncon=i32([p[1] for p in T.pairs]), pair_dst=i32(T.pair_dst),
        con_dim=i32(T.con_dim), con_geom1=i32(T.con_geom1), con_geom2=i32(T.con_geom2), con_efc_address=i32(T.con_efc_address),
        convex_nvert=i32([]), convex_nface=i32([]), convex_nfv=i32([]), convex_nedge=i32([]), convex_vertadr=i32([]),
        convex_faceadr=i32([]), convex_normadr=i32([]), convex_edgeadr=i32([]), convex_face=i32([]), convex_edge=i32([]),
    )
    # convex tables (box / mesh geoms): one record per convex geom, flat arrays with offsets
    cv = [(g, c) for g, c in enumerate(T.convex) if c is not None]
    convexid = -np.ones(m.ngeom, dtype=np.int32)
    for i, (g, _) in enumerate(cv):
        convexid[g] = i
    off = lambda ns: np.concatenate([[0], np.cumsum(ns)[:-1]]) if ns else []
    int_arrays.update(
        geom_convexid=convexid, convex_nvert=i32([len(c["vert"]) for _, c in cv]), convex_nface=i32([c["face"].shape[0] for _, c in cv]),
        convex_nfv=i32([c["face"].shape[1] for _, c in cv]), convex_nedge=i32([len(c["edge"]) for _, c in cv]),
        convex_vertadr=i32(off([len(c["vert"]) for _, c in cv])), convex_faceadr=i32(off([c["face"].size for _, c in cv])),
        convex_normadr=i32(off([c["face"].shape[0] for _, c in cv])), convex_edgeadr=i32(off([len(c["edge"]) for _, c in cv])),
        convex_face=i32(np.concatenate([c["face"].reshape(-1) for _, c in cv]) if cv else []),
        convex_edge=i32(np.concatenate([c["edge"].reshape(-1) for _, c in cv]) if cv else []),
    )
    ints["nconvex"] = len(cv)
    st = static_contact_fields(model_float_leaves(m, dtype), T, dtype)
    empty = np.zeros(0)
    cvf = lambda k: f64(torch.tensor(np.concatenate([c[k].reshape(-1) for _, c in cv]))) if cv else empty
    real_arrays = dict(
        qpos0=f64(m.qpos0), qpos_spring=f64(m.qpos_spring), body_pos=f64(m.body_pos), body_quat=f64(m.body_quat),
        body_ipos=f64(m.body_ipos), body_iquat=f64(m.body_iquat), body_mass=f64(m.body_mass),
        body_inertia=f64(m.body_inertia), body_invweight0=f64(m.body_invweight0[:, 0]), jnt_pos=f64(m.jnt_pos),
        jnt_axis=f64(m.jnt_axis), jnt_stiffness=f64(m.jnt_stiffness), jnt_range=f64(m.jnt_range),
        jnt_margin=f64(m.jnt_margin), jnt_solref=f64(m.jnt_solref), jnt_solimp=f64(m.jnt_solimp),
        jnt_actfrcrange=f64(m.jnt_actfrcrange), dof_armature=f64(m.dof_armature), dof_damping=f64(m.dof_damping),
        dof_invweight0=f64(m.dof_invweight0), sns_cutoff=f64(torch.tensor(np.asarray(T.sensors["cutoff"], dtype=np.float64))), dof_frictionloss=f64(m.dof_frictionloss), dof_solref=f64(m.dof_solref), dof_solimp=f64(m.dof_solimp),
        **_tendon_reals(src, T, dtype), body_gravcomp=f64(m.body_gravcomp), body_invweight0_rot=f64(m.body_invweight0[:, 1]), eq_data=f64(m.eq_data) if m.neq else empty, eq_solref=f64(m.eq_solref) if m.neq else empty, eq_solimp=f64(m.eq_solimp) if m.neq else empty,
        geom_pos=f64(m.geom_pos), geom_quat=f64(m.geom_quat),
        geom_size=f64(m.geom_size), site_pos=f64(m.site_pos), site_quat=f64(m.site_quat), cam_pos=f64(m.cam_pos),
        cam_quat=f64(m.cam_quat), cam_pos0=f64(m.cam_pos0), cam_mat0=f64(m.cam_mat0), light_pos=f64(m.light_pos),
        light_dir=f64(m.light_dir), act_gear=f64(m.actuator_gear) if nu else empty,
        act_gainprm=f64(m.actuator_gainprm[:, :9]) if nu else empty, act_biasprm=f64(m.actuator_biasprm[:, :9]) if nu else empty,
        act_lengthrange=f64(m.actuator_lengthrange) if nu else empty, act_acc0=f64(m.actuator_acc0) if nu else empty,
        act_dynprm=f64(m.actuator_dynprm[:, :3]) if nu else empty, act_ctrlrange=f64(m.actuator_ctrlrange) if nu else empty,
        act_forcerange=f64(m.actuator_forcerange) if nu else empty, act_actrange=f64(m.actuator_actrange) if nu else empty,
        con_includemargin=f64(st["includemargin"]), con_friction=f64(st["friction"]), con_solref=f64(st["solref"]),
        con_solreffriction=f64(st["solreffriction"]), con_solimp=f64(st["solimp"]), convex_vert=cvf("vert"), convex_facenormal=cvf("facenormal"),
    )
    desc = ModelDesc()
    desc.abi_version = ABI_VERSION
    keep = []
    for n in LISTS["MJH_MODEL_INTS"]:
        setattr(desc, n, int(ints[n]))
    for n in LISTS["MJH_MODEL_REALS"]:
        setattr(desc, n, float(reals[n]))
    for n in LISTS["MJH_MODEL_INT_ARRAYS"]:
        a = int_arrays[n]
        keep.append(a)
        setattr(desc, n, a.ctypes.data if a.size else None)
        setattr(desc, "len_" + n, a.size)
    for n in LISTS["MJH_MODEL_REAL_ARRAYS"]:
        a = np.ascontiguousarray(real_arrays[n], dtype=np.float64)
        keep.append(a)
        setattr(desc, n, a.ctypes.data if a.size else None)
        setattr(desc, "len_" + n, a.size)
    return desc, keep


def data_field_tensor(d, name):
    obj = d
    for p in DATA_PATH[name]:
        obj = getattr(obj, p)
    return obj


_lib = None


class RayCands(ctypes.Structure):
    """include/mjhip.h mjhRayCands: the candidate geoms of one mjh_ray call (device pointers)."""

    _fields_ = [("ncand", ctypes.c_int64), ("cand", ctypes.c_void_p), ("tri", ctypes.c_void_p), ("geom_size", ctypes.c_void_p)]


class RenderScene(ctypes.Structure):
    """include/mjhip.h mjhRenderScene: the scene tables of one mjh_render call (device pointers)."""

    _fields_ = [("ncand", ctypes.c_int64), ("nprim", ctypes.c_int64), ("cand", ctypes.c_void_p), ("tri", ctypes.c_void_p), ("geom_size", ctypes.c_void_p),
                ("geom_rgba", ctypes.c_void_p), ("geom_matid", ctypes.c_void_p), ("mat_rgba", ctypes.c_void_p), ("nlight", ctypes.c_int64),
                ("light", ctypes.c_void_p)]


class RenderParams(ctypes.Structure):
    """include/mjhip.h mjhRenderParams: one mjh_render call's settings."""

    _fields_ = [(n, ctypes.c_int32) for n in ("camera", "width", "height", "ssaa", "shading", "shadows", "fog", "rgb_f32", "u8", "reserved")] + [
        ("half_w", ctypes.c_double), ("half_h", ctypes.c_double), ("background", ctypes.c_double * 3), ("fog_color", ctypes.c_double * 3),
        ("fog_start", ctypes.c_double), ("fog_range", ctypes.c_double)]


class SupportArgs(ctypes.Structure):
    """include/mjhip.h mjhSupportArgs: one mjh_support call (device pointers, element strides)."""

    _fields_ = [("op", ctypes.c_int32), ("P", ctypes.c_int32), ("K", ctypes.c_int32), ("reserved", ctypes.c_int32), ("B", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("cdof", "subtree_com", "xipos", "xfrc_applied", "qM", "qLD", "body_id")] + [("body_stride", ctypes.c_int64)] + [
        f for n in ("point", "force", "torque") for f in ((n, ctypes.c_void_p), (n + "_env", ctypes.c_int64), (n + "_q", ctypes.c_int64))] + [
        ("vec", ctypes.c_void_p), ("vec_env", ctypes.c_int64), ("vec_k", ctypes.c_int64), ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p)]


class PostconArgs(ctypes.Structure):
    """include/mjhip.h mjhPostconArgs: one mjh_postconstraint call (device pointers)."""

    _fields_ = [("flags", ctypes.c_int32), ("reserved", ctypes.c_int32), ("B", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "qvel", "qacc", "cdof", "cdof_dot", "cvel", "cinert", "xipos", "ximat", "subtree_com", "xfrc_applied", "efc_force", "contact_pos", "contact_frame",
        "contact_friction", "contact_dim", "contact_geom", "contact_efc_address", "site_xpos", "site_xmat", "sensordata_in", "body_subtreemass", "cacc", "cfrc_int",
        "cfrc_ext", "subtree_linvel", "subtree_angmom", "sensordata")]


class ContactSensorArgs(ctypes.Structure):
    """include/mjhip.h mjhContactSensorArgs: one mjh_contact_sensors call (device pointers)."""

    _fields_ = [("flags", ctypes.c_int32), ("nsens", ctypes.c_int32), ("B", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "efc_force", "contact_pos", "contact_frame", "contact_friction", "contact_dim", "contact_geom", "contact_efc_address", "site_xpos", "site_xmat", "cvel", "cacc",
        "subtree_com", "xipos", "xpos", "geom_xpos", "cam_xpos", "site_size", "sns", "sns_cutoff", "force", "sensordata")]


class EnergyArgs(ctypes.Structure):
    """include/mjhip.h mjhEnergyArgs: one mjh_energy call (device pointers)."""

    _fields_ = [("flags", ctypes.c_int32), ("nsens", ctypes.c_int32), ("B", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "qpos", "qvel", "xipos", "ten_length", "qM", "efc_J", "efc_force", "gravity", "body_mass", "jnt_stiffness", "qpos_spring", "jnt_range", "jnt_margin",
        "tendon_stiffness", "tendon_lengthspring", "tendon_range", "tendon_margin", "sns", "sns_cutoff", "energy", "sensordata")]


class IntegrateArgs(ctypes.Structure):
    """include/mjhip.h mjhIntegrateArgs: one mjh_integrate call (device pointers)."""

    _fields_ = [("flags", ctypes.c_int32), ("disableflags", ctypes.c_int32), ("B", ctypes.c_int64), ("h", ctypes.c_double), ("gain_stride", ctypes.c_int32),
                ("bias_stride", ctypes.c_int32), ("dyn_stride", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in (
        "qpos", "qvel", "act", "act_dot", "time", "ctrl", "qacc", "qM", "qfrc_smooth", "qfrc_constraint", "actuator_moment", "ten_J", "dof_damping", "tendon_damping",
        "gainprm", "biasprm", "dynprm", "actrange", "qpos_out", "qvel_out", "act_out", "time_out", "qderiv_out", "qacc_out")]


class JacobianArgs(ctypes.Structure):
    """include/mjhip.h mjhJacobianArgs: one mjh_jacobian call (device pointers, element strides)."""

    _fields_ = [("op", ctypes.c_int32), ("P", ctypes.c_int32), ("B", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "cdof", "cdof_dot", "cvel", "subtree_com", "xipos", "ximat", "body_mass", "body_subtreemass", "body_inertia", "body_id")] + [
        ("body_stride", ctypes.c_int64), ("point", ctypes.c_void_p), ("point_env", ctypes.c_int64), ("point_q", ctypes.c_int64), ("vec", ctypes.c_void_p),
        ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p)]


class ConstraintSpaceArgs(ctypes.Structure):
    """include/mjhip.h mjhConstraintSpaceArgs: one mjh_constraint_space call (device pointers, element strides).  Bound below like ``mjh_ray`` and its
    ``RayCands``, beside the ``ARGS`` table (tests/test_constraint_space_host.py compares it with the header)."""

    _fields_ = [("op", ctypes.c_int32), ("K", ctypes.c_int32), ("ne_nf", ctypes.c_int32), ("floss", ctypes.c_int32), ("B", ctypes.c_int64),
                ("meaninertia", ctypes.c_double)] + [(n, ctypes.c_void_p) for n in (
        "efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qM", "qLD", "qfrc_smooth", "qacc_smooth", "qacc", "jar_in", "vec")] + [
        ("vec_env", ctypes.c_int64), ("vec_k", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "out", "jar", "efc_force", "efc_state", "qfrc_constraint", "cost", "gauss", "grad", "grad_norm", "AR", "b")]


class PgsArgs(ctypes.Structure):
    """include/mjhip.h mjhPgsArgs: one mjh_pgs call (device pointers, an element stride).  Bound below beside the ``ARGS`` table, like ``ConstraintSpaceArgs``
    (tests/test_pgs_host.py compares it with the header)."""

    _fields_ = [("ne", ctypes.c_int32), ("nf", ctypes.c_int32), ("iterations", ctypes.c_int32), ("pad_", ctypes.c_int32), ("B", ctypes.c_int64),
                ("meaninertia", ctypes.c_double), ("tolerance", ctypes.c_double)] + [(n, ctypes.c_void_p) for n in (
        "efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "force0")] + [("force0_env", ctypes.c_int64)] + [(n, ctypes.c_void_p) for n in (
        "efc_force", "qfrc_constraint", "qacc", "cost", "improvement", "niter")]


class NoslipArgs(ctypes.Structure):
    """include/mjhip.h mjhNoslipArgs: one mjh_noslip call (device pointers, an element stride).  Bound below beside the ``ARGS`` table, like ``PgsArgs``
    (tests/test_noslip_host.py compares it with the header)."""

    _fields_ = [("ne", ctypes.c_int32), ("nf", ctypes.c_int32), ("iterations", ctypes.c_int32), ("pad_", ctypes.c_int32), ("B", ctypes.c_int64),
                ("meaninertia", ctypes.c_double), ("tolerance", ctypes.c_double)] + [(n, ctypes.c_void_p) for n in (
        "efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qLD", "qacc_smooth", "force0", "contact_friction")] + [("force0_env", ctypes.c_int64)] + [
        (n, ctypes.c_void_p) for n in ("efc_force", "qfrc_constraint", "qacc", "cost", "improvement", "niter")]


class SolveArgs(ctypes.Structure):
    """include/mjhip.h mjhSolveArgs: one mjh_solve call (device pointers).  Bound below beside the ``ARGS`` table, like ``PgsArgs`` (tests/test_solve_host.py
    compares it with the header)."""

    _fields_ = [(n, ctypes.c_int32) for n in ("ne", "nf", "floss", "solver", "iterations", "ls_iterations", "fixed", "warmstart")] + [("B", ctypes.c_int64)] + [
        (n, ctypes.c_double) for n in ("tolerance", "ls_tolerance", "meaninertia")] + [(n, ctypes.c_void_p) for n in (
        "efc_J", "efc_D", "efc_aref", "efc_frictionloss", "qM", "qLD", "qfrc_smooth", "qacc_smooth", "qacc_warmstart", "qacc_out", "qacc_warmstart_out",
        "qfrc_constraint_out", "efc_force_out", "cost", "improvement", "grad_norm", "niter")]


class SmoothArgs(ctypes.Structure):
    """include/mjhip.h mjhSmoothArgs: one mjh_smooth call (device pointers).  Bound below beside the ``ARGS`` table, like ``SolveArgs`` (tests/test_smooth_host.py
    compares it with the header, field by field, with tests/test_abi.py's own parser)."""

    _fields_ = [(n, ctypes.c_int32) for n in ("op", "flg_acc", "disableflags", "reserved")] + [("B", ctypes.c_int64)] + [
        (n, ctypes.c_double) for n in ("gravity_x", "gravity_y", "gravity_z")] + [(n, ctypes.c_void_p) for n in (
        "xipos", "ximat", "xmat", "xanchor", "xaxis", "cinert", "cdof", "cdof_dot", "cvel", "qvel", "qacc", "qM", "ten_J", "body_mass", "body_inertia", "dof_armature",
        "tendon_armature", "subtree_com_out", "cinert_out", "cdof_out", "crb_out", "qM_out", "qLD_out", "cvel_out", "cdof_dot_out", "qfrc_bias_out")]


class DynamicsArgs(ctypes.Structure):
    """include/mjhip.h mjhDynamicsArgs: one mjh_dynamics call (device pointers).  Bound below beside the ``ARGS`` table, like ``SmoothArgs`` (tests/test_dynamics_host.py
    compares it with the header, field by field, with tests/test_abi.py's own parser)."""

    _fields_ = [(n, ctypes.c_int32) for n in ("op", "disableflags", "has_gravcomp", "has_fluid", "gain_stride", "bias_stride", "dyn_stride", "reserved")] + [
        ("B", ctypes.c_int64)] + [(n, ctypes.c_double) for n in ("gravity_x", "gravity_y", "gravity_z", "wind_x", "wind_y", "wind_z", "density", "viscosity")] + [
        (n, ctypes.c_void_p) for n in (
            "qpos", "qvel", "ctrl", "act", "ten_length", "ten_velocity", "ten_J", "actuator_length", "actuator_velocity", "actuator_moment", "xipos", "ximat", "subtree_com",
            "cdof", "cvel", "qfrc_gravcomp", "qfrc_applied", "xfrc_applied", "qfrc_passive", "qfrc_bias", "qfrc_actuator", "qLD", "jnt_stiffness", "qpos_spring",
            "dof_damping", "tendon_stiffness", "tendon_damping", "tendon_lengthspring", "body_mass", "body_inertia", "body_gravcomp", "jnt_actgravcomp", "jnt_actfrcrange",
            "gainprm", "biasprm", "dynprm", "ctrlrange", "forcerange", "gear", "lengthrange", "acc0", "ten_length_out", "ten_J_out", "actuator_length_out",
            "actuator_moment_out", "actuator_velocity_out", "ten_velocity_out", "qfrc_passive_out", "qfrc_gravcomp_out", "act_dot_out", "qfrc_actuator_out",
            "actuator_force_out", "qfrc_smooth_out", "qacc_smooth_out")]


# the entry points that take (handle, args struct, stream): symbol -> the struct (tests/test_abi.py compares every struct with the header)
ARGS = {"mjh_support": SupportArgs, "mjh_postconstraint": PostconArgs, "mjh_contact_sensors": ContactSensorArgs, "mjh_energy": EnergyArgs,
        "mjh_integrate": IntegrateArgs, "mjh_jacobian": JacobianArgs}


def load_library(path: str | None = None):
    """Loads libmjhip.so (once). Raises if it has not been built: no fallback path exists."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"native stepper library not found at {p}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). mujoco_torch_amd has no CPU / PyTorch fallback."
        )
    lib = ctypes.CDLL(p)
    lib.mjh_model_create.argtypes = [ctypes.POINTER(ModelDesc), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.mjh_model_create.restype = ctypes.c_int
    lib.mjh_model_destroy.argtypes = [ctypes.c_void_p]
    lib.mjh_model_destroy.restype = None
    lib.mjh_forward.argtypes = [ctypes.c_void_p, ctypes.POINTER(DataPtrs), ctypes.POINTER(DataPtrs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.mjh_forward.restype = ctypes.c_int
    lib.mjh_step.argtypes = [ctypes.c_void_p, ctypes.POINTER(DataPtrs), ctypes.POINTER(DataPtrs), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    lib.mjh_step.restype = ctypes.c_int
    lib.mjh_inverse.argtypes = [ctypes.c_void_p, ctypes.POINTER(DataPtrs), ctypes.POINTER(DataPtrs), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    lib.mjh_inverse.restype = ctypes.c_int
    if hasattr(lib, "mjh_ray"):  # (a build from before ray casting still binds everything else: tools/bitcmp.py steps a parent's library)
        lib.mjh_ray.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(RayCands), ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p]
        lib.mjh_ray.restype = ctypes.c_int
    if hasattr(lib, "mjh_render"):  # (likewise a build from before rendering)
        lib.mjh_render.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.POINTER(RenderScene), ctypes.POINTER(RenderParams),
                                                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.mjh_render.restype = ctypes.c_int
    if hasattr(lib, "mjh_geom_distance"):  # (likewise a build from before geom distances)
        lib.mjh_geom_distance.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        lib.mjh_geom_distance.restype = ctypes.c_int
    if hasattr(lib, "mjh_qpos_arith"):  # (likewise a build from before the configuration arithmetic and the site IK)
        lib.mjh_qpos_arith.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
        lib.mjh_qpos_arith.restype = ctypes.c_int
    if hasattr(lib, "mjh_ik_site_step"):
        lib.mjh_ik_site_step.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                                                   ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int,
                                                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                                                   ctypes.c_void_p]
        lib.mjh_ik_site_step.restype = ctypes.c_int
    for symbol, struct in ARGS.items():
        if hasattr(lib, symbol):  # (likewise a build from before that entry point)
            fn = getattr(lib, symbol)
            fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(struct), ctypes.c_void_p]
            fn.restype = ctypes.c_int
    if hasattr(lib, "mjh_constraint_space"):  # (likewise a build from before the constraint-space functions)
        lib.mjh_constraint_space.argtypes = [ctypes.c_void_p, ctypes.POINTER(ConstraintSpaceArgs), ctypes.c_void_p]
        lib.mjh_constraint_space.restype = ctypes.c_int
        lib.mjh_constraint_space_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_constraint_space_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_pgs"):  # (likewise a build from before solve_pgs)
        lib.mjh_pgs.argtypes = [ctypes.c_void_p, ctypes.POINTER(PgsArgs), ctypes.c_void_p]
        lib.mjh_pgs.restype = ctypes.c_int
        lib.mjh_pgs_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_pgs_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_noslip"):  # (likewise a build from before solve_noslip)
        lib.mjh_noslip.argtypes = [ctypes.c_void_p, ctypes.POINTER(NoslipArgs), ctypes.c_void_p]
        lib.mjh_noslip.restype = ctypes.c_int
        lib.mjh_noslip_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_noslip_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_solve"):  # (likewise a build from before solve)
        lib.mjh_solve.argtypes = [ctypes.c_void_p, ctypes.POINTER(SolveArgs), ctypes.c_void_p]
        lib.mjh_solve.restype = ctypes.c_int
        lib.mjh_solve_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_solve_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_smooth"):  # (likewise a build from before the smooth-dynamics functions)
        lib.mjh_smooth.argtypes = [ctypes.c_void_p, ctypes.POINTER(SmoothArgs), ctypes.c_void_p]
        lib.mjh_smooth.restype = ctypes.c_int
        lib.mjh_smooth_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_smooth_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_dynamics"):  # (likewise a build from before tendon .. fwd_acceleration)
        lib.mjh_dynamics.argtypes = [ctypes.c_void_p, ctypes.POINTER(DynamicsArgs), ctypes.c_void_p]
        lib.mjh_dynamics.restype = ctypes.c_int
        lib.mjh_dynamics_plan.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)]
        lib.mjh_dynamics_plan.restype = ctypes.c_int
    if hasattr(lib, "mjh_integrate_plan"):
        lib.mjh_integrate_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        lib.mjh_integrate_plan.restype = ctypes.c_int
    lib.mjh_reset_where.argtypes = [ctypes.c_void_p, ctypes.POINTER(DataPtrs), ctypes.POINTER(DataPtrs), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.mjh_reset_where.restype = ctypes.c_int
    lib.mjh_debug_phase_timing.argtypes = [ctypes.c_int]
    lib.mjh_debug_phase_timing.restype = ctypes.c_int
    lib.mjh_debug_phase_times.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.mjh_debug_phase_times.restype = ctypes.c_int
    lib.mjh_model_lds_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.mjh_model_lds_bytes.restype = ctypes.c_int
    lib.mjh_model_work_bytes.argtypes = [ctypes.c_void_p]
    lib.mjh_model_work_bytes.restype = ctypes.c_int64
    lib.mjh_model_kernel_io.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    lib.mjh_model_kernel_io.restype = ctypes.c_int
    lib.mjh_model_leaf_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    lib.mjh_model_leaf_counts.restype = ctypes.c_int
    for fn in ("mjh_last_error", "mjh_data_fields", "mjh_model_fields"):
        getattr(lib, fn).restype = ctypes.c_char_p
    lib.mjh_abi_version.restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


def check_abi(lib):
    """Asserts the header this binding was generated from matches the loaded library."""
    data = lib.mjh_data_fields().decode().split(",")
    want = LISTS["MJH_DATA_REALS"] + LISTS["MJH_DATA_I32"] + LISTS["MJH_DATA_I64"]
    if data != want:
        raise RuntimeError("libmjhip.so Data field list does not match include/mjhip.h")
    lib.mjh_data_extra_fields.restype = ctypes.c_char_p
    if lib.mjh_data_extra_fields().decode().split(",") != LISTS["MJH_DATA_EXTRA_IN"] or int(lib.mjh_sizeof_data()) != ctypes.sizeof(DataPtrs):
        raise RuntimeError("libmjhip.so mjhData layout (trailing input-only leaves) does not match include/mjhip.h")
    model = lib.mjh_model_fields().decode().split(",")
    wantm = LISTS["MJH_MODEL_INTS"] + LISTS["MJH_MODEL_REALS"] + LISTS["MJH_MODEL_INT_ARRAYS"] + LISTS["MJH_MODEL_REAL_ARRAYS"]
    if model != wantm:
        raise RuntimeError("libmjhip.so Model field list does not match include/mjhip.h")


class NativeModel:
    """Device-resident constant blob for one (device, dtype) and one set of model VALUES."""

    def __init__(self, desc, keep, device: torch.device, dtype: torch.dtype):
        # `keep`: the host arrays `desc` points into; the library copies them into its device blob, nothing is retained
        self.lib = load_library()
        check_abi(self.lib)
        handle = ctypes.c_void_p()
        with torch.cuda.device(device):
            rc = self.lib.mjh_model_create(ctypes.byref(desc), MJH_F64 if dtype == torch.float64 else MJH_F32, ctypes.byref(handle))
        if rc != 0:
            raise RuntimeError(f"mjh_model_create failed ({rc}): {self.lib.mjh_last_error().decode()}")
        self.handle = handle
        self.device = device
        self.dtype = dtype
        self.work_bytes = int(self.lib.mjh_model_work_bytes(handle))
        self.lds_bytes = [int(self.lib.mjh_model_lds_bytes(handle, p)) for p in range(6)]  # five phases + the register solver's arena
        n = len(DATA_PATH)
        buf = (ctypes.c_int64 * n)()
        got = int(self.lib.mjh_model_leaf_counts(handle, buf, n))
        if got != n:
            raise RuntimeError("libmjhip.so leaf table does not match include/mjhip.h")
        self.leaf_counts = np.array(list(buf), dtype=np.int64)  # per-environment element count of every Data leaf, ABI order
        self._work = {"clock": 0, "bufs": {}}  # replaced by the pool shared through the tables object (get_native_model): the LRU clock lives WITH the pool

    def workspace(self, B: int, stream: int = 0):
        """Scratch for RK4 (stage Data + running sums), one per (batch size, stream): two streams stepping the same model
        must not share stage storage, and a buffer is only ever reused on the stream it was allocated on."""
        if self.work_bytes == 0:
            return None
        key = (B, stream)
        pool = self._work
        bufs = pool["bufs"]
        pool["clock"] += 1  # one clock per pool: every blob of a tables object ages the entries on the same scale (a per-blob clock made a new blob's fresh entries look oldest)
        hit = bufs.get(key)
        if hit is not None:
            hit[1] = pool["clock"]
            return hit[0]
        if len(bufs) >= 4:  # small LRU: ping-pong between a few batch sizes / streams without re-allocating
            del bufs[min(bufs, key=lambda k: bufs[k][1])]
        w = torch.empty(self.work_bytes * B, dtype=torch.uint8, device=self.device)
        bufs[key] = [w, pool["clock"]]
        return w

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.mjh_model_destroy(self.handle)
        except Exception:
            pass


# option bits that decide the STATIC tables built by device_put (row counts, contact list, sensor list): changing them on a
# Model after device_put would need new tables and a new Data layout (the reference's own constraint_sizes_py goes stale too)
_STRUCT_DISABLE = 0b11111 | (1 << 13)  # CONSTRAINT, EQUALITY, FRICTIONLOSS, LIMIT, CONTACT, SENSOR


def _structure_key(opt):
    return (int(opt.cone), int(opt.disableflags) & _STRUCT_DISABLE, int(opt.jacobian))


def _stamp(m):
    """Cheap per-call check that nothing pack_model reads has changed since the blob was cached ON THIS CONTAINER: container
    versions (update_ / attribute assignment) and the in-place version counters of every tensor leaf pack_model reads -- Model,
    opt and stat (``stat.meaninertia`` is packed), plain or wrapped in an ``UnbatchedTensor``.  The opt / stat containers are
    compared by identity through references held in the cache entry (an ``id()`` can be reused after garbage collection)."""
    opt, stat = m.opt, m.stat
    v = 0
    for c in (m, opt, stat):
        # the tensor leaves of a container only change with its version (attribute assignment / update_): the list is kept per container and version, so a
        # step pays one `_version` read per tensor instead of walking ~450 fields through isinstance (45 of the host's 110 us per call)
        d = c.__dict__
        ver = d.get("_ver", 0)
        ts = d.get("_stamp_ts")
        if ts is not None and ts[0] == ver:
            for w, t0 in ts[2]:
                if w.data is not t0:  # `unbatched.data = new_tensor` bumps no version counter: the wrapper is re-read every call
                    ts = (ver, None, None, ts[3] + 1)
                    break
        if ts is None or ts[0] != ver or ts[1] is None:
            lst, wrapped = [], []
            for t in c._fields.values():
                if isinstance(t, UnbatchedTensor):
                    if isinstance(t.data, torch.Tensor):
                        wrapped.append((t, t.data))
                    t = t.data
                if isinstance(t, torch.Tensor):
                    lst.append(t)
            ts = (ver, lst, wrapped, ts[3] if ts is not None else 0)
            object.__setattr__(c, "_stamp_ts", ts)
        v += ts[3] << 32
        for t in ts[1]:
            v += t._version
    return (m.__dict__.get("_ver", 0), opt, opt.__dict__.get("_ver", 0), stat, stat.__dict__.get("_ver", 0), v)


def _same_stamp(a, b):
    return a[0] == b[0] and a[1] is b[1] and a[2] == b[2] and a[3] is b[3] and a[4] == b[4] and a[5] == b[5]


_NATIVE_LRU = 4  # blobs the shared tables keep alive on their own (most recently used); every Model also holds the one it stepped


def _desc_digest(desc, keep):
    import hashlib

    h = hashlib.blake2b(digest_size=16)
    h.update(bytes(memoryview(desc))[: ModelDesc.__dict__[LISTS["MJH_MODEL_INT_ARRAYS"][0]].offset])  # the scalar head: ints and reals
    for a in keep:
        h.update(a.dtype.str.encode())
        h.update(np.int64(a.size).tobytes())
        h.update(a.tobytes())
    return h.digest()


def get_native_model(m, device: torch.device, dtype: torch.dtype) -> NativeModel:
    """The device blob for this Model's CURRENT values.  Blobs are shared through ``m.tables.native`` keyed by a digest of
    everything ``pack_model`` hands to the library, so ``mx.replace(body_mass=...)`` / ``mx.tree_replace({'opt.timestep': ..})``
    (reference test/smooth_test.py:204) get a blob of their own while ``mx.to(...)`` copies share one."""
    key = (device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else -1), dtype)
    stamp = _stamp(m)
    local = m.__dict__.get("_native_cache")
    if local is not None:
        hit = local.get(key)
        if hit is not None and _same_stamp(hit[0], stamp):
            return hit[1]
    T = m.tables
    built = getattr(T, "structure_key", None)
    if built is not None and _structure_key(m.opt) != built:
        raise NotImplementedError(
            "opt.cone / opt.jacobian / the constraint-, contact- or sensor-disabling bits of opt.disableflags changed after "
            "device_put: they size the static row and contact tables (and the Data layout).  Set them on the source model and "
            "call device_put again.")
    desc, keep = pack_model(m, dtype)
    shared_key = (key, _desc_digest(desc, keep))
    nm = T.native.get(shared_key)
    if nm is None:
        nm = NativeModel(desc, keep, torch.device(device.type, key[0]) if key[0] >= 0 else device, dtype)
        # RK4 workspaces are sized by the model's STRUCTURE (leaf counts), not its values: one pool per tables object and (device, dtype), so
        # per-episode domain randomisation (mx.replace(body_mass=...)) re-uses the same scratch instead of growing a pool per blob
        nm._work = T.__dict__.setdefault("_workspaces", {}).setdefault((key, nm.work_bytes), {"clock": 0, "bufs": {}})
        T.native[shared_key] = nm
    # T.native holds blobs weakly: one lives as long as a Model that stepped it (its _native_cache) does, so `mx.replace(body_mass=...)` per
    # episode frees the previous episode's blob with its Model instead of leaking device memory.  The few most recently used ones are also
    # held strongly, so alternating between a handful of value sets through fresh `replace` results does not rebuild every time.
    recent = T.native_recent
    recent.pop(shared_key, None)
    recent[shared_key] = nm
    while len(recent) > _NATIVE_LRU:
        recent.popitem(last=False)
    if local is None:
        local = {}
        object.__setattr__(m, "_native_cache", local)
    local[key] = (stamp, nm)
    return nm
