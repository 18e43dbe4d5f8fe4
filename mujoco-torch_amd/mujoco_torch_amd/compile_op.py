"""``step`` / ``forward`` as a ``torch.library`` custom operator over the flat list of Data leaves.

Why: the reference's published batched mode is ``torch.compile(torch.vmap(lambda d: step(mx, d)), fullgraph=True)``
(``benchmarks/bench_compile.py:39-43``).  The native step is one opaque launch sequence: nothing in it can be traced, and under
``fullgraph=True`` nothing may graph-break either.  So when ``step`` is reached by Dynamo, or its Data holds functorch batched tensors
(plain ``torch.vmap``), it calls ``torch.ops.mujoco_torch_amd.step_leaves`` instead of the ctypes path:

* the operator takes the Data leaves in ABI order (``include/mjhip.h`` X-macro lists, then the input-only ``MJH_DATA_EXTRA_IN`` leaves; an absent leaf is an empty tensor), the Model as a
  process-unique number in a 0-dim int64 TENSOR (``Model._op_key_t``, resolved through a weak registry -- an operator cannot take a container; as a tensor it is an
  input of a traced graph, so ``mx.replace(body_mass=...)`` per episode steps the new values WITHOUT a recompile), the structure id ``tables.uid`` as a string (the
  graph's constant: shape propagation runs on any Model of that structure) and the call's flags; it returns the leaves the call writes, in ``forward._written_names`` order;
* its eager implementation rebuilds a ``Data`` around the tensors and runs the very same ``forward._run`` (the native batch);
* ``register_fake`` gives the output shapes (batch dims of ``qpos`` + the per-environment shape of each leaf), so Inductor / AOT see an
  ordinary opaque node;
* ``register_vmap`` maps a vmapped call onto ONE native batch: batched leaves move their mapped dimension to the front, unmapped ones are
  broadcast, outputs carry the mapped dimension first.  No private functorch call is involved.

The fast path of a direct ``step(mx, d)`` on plain tensors does not go through the operator (forward.py).

``inverse`` has an operator of its own, ``torch.ops.mujoco_torch_amd.inverse_leaves``: the same leaves in, the leaves an inverse call writes
(``forward._inverse_names``) and then ``qfrc_inverse`` out, with the same fake and vmap rules.
"""

from __future__ import annotations

import torch

from . import native
from .types import _MODELS_BY_KEY, structure_model

_NAMES = native.LISTS["MJH_DATA_REALS"] + native.LISTS["MJH_DATA_I32"] + native.LISTS["MJH_DATA_I64"]
_NREAL = len(native.LISTS["MJH_DATA_REALS"])
_INT_DTYPE = {n: torch.int32 for n in native.LISTS["MJH_DATA_I32"]} | {n: torch.int64 for n in native.LISTS["MJH_DATA_I64"]}
_QPOS = _NAMES.index("qpos")
# Input-only leaves that trail the ABI struct (cacc, cfrc_int, subtree_linvel, subtree_angmom: no stage writes them, sensors read them --
# include/mjhip.h MJH_DATA_EXTRA_IN).  They ride behind the ABI leaves in the operator's list so that a vmapped / traced call hands the
# CALLER's batched values to the native step (rebuilt from the unbatched template they failed the size check and were dropped).
_XNAMES = native.LISTS["MJH_DATA_EXTRA_IN"]
_TEMPLATES = {}  # tables uid -> an unbatched make_data(m): the fields outside the ABI and the per-environment shape of every leaf


def _model(key) -> "Model":
    """The Model whose VALUES this call steps: the operator receives its process-unique number as a 0-dim int64 tensor (an input of the traced graph, not a constant)."""
    m = _MODELS_BY_KEY.get(int(key))
    if m is None:
        raise RuntimeError("mujoco_torch_amd::step_leaves: the Model this call was made with no longer exists")
    return m


def _structure(uid: str):
    """Any live Model of that structure (tables.uid, as the string the graph carries: an int that changes between calls is made a symbolic
    shape by Dynamo's automatic dynamism, a string stays a guarded constant): what shape propagation needs does not depend on values."""
    m = structure_model(uid)
    if m is None:
        raise RuntimeError("mujoco_torch_amd::step_leaves: no Model of the structure this call was traced with exists any more")
    return m


def _template(m):
    from .io import make_data

    uid = m.tables.uid
    t = _TEMPLATES.get(uid)
    if t is None:
        if len(_TEMPLATES) > 64:
            _TEMPLATES.clear()
        from torch._subclasses.fake_tensor import unset_fake_temporarily

        with unset_fake_temporarily():  # first needed while an operator call is being shape-propagated: real tensors, outside the fake mode
            t = _TEMPLATES[uid] = make_data(m)
    return t


def out_names(m, do_step: bool, stages: int):
    """The leaves one call writes (what the operator returns, in this order)."""
    from .forward import _written_names  # (the package attribute `forward` is the function, not the module)

    names = _written_names(m, do_step)
    if not do_step and not (stages & 0x40):
        names = [n for n in names if n != "sensordata"]
    return names


def inverse_out_names(m):
    """The leaves one inverse call writes, then qfrc_inverse (what ``inverse_leaves`` returns, in this order)."""
    from .forward import _inverse_names

    return _inverse_names(m) + ["qfrc_inverse"]


def _leaf_of(tmpl, n):
    return tmpl.qfrc_inverse if n == "qfrc_inverse" else native.data_field_tensor(tmpl, n)


def _data_of_leaves(m, leaves):
    """The Data the operator's eager implementation runs on: the template with the caller's leaves put in."""
    tmpl = _template(m)
    top, con = {n: None for n in _XNAMES}, {}  # an absent input-only leaf is NULL (zeros) for the kernels -- never the template's unbatched copy
    for n, t in zip(_XNAMES, leaves[len(_NAMES):]):
        if t.numel() != 0:
            top[n] = t
    for n, t in zip(_NAMES, leaves):
        if t.numel() == 0 and t.dim() == 1 and native.data_field_tensor(tmpl, n) is not None and native.data_field_tensor(tmpl, n).numel() != 0:
            continue  # placeholder of a leaf the caller's Data did not carry: keep the template's
        path = native.DATA_PATH[n]
        (con if len(path) == 2 else top)[path[-1]] = t
    batch = tuple(leaves[_QPOS].shape[:-1])
    d = tmpl.replace(contact=tmpl.contact.replace(**con), **top)
    object.__setattr__(d, "_bs", batch)
    object.__setattr__(d.contact, "_bs", batch)
    return d


def _destination(m, d, leaves, names):
    """(fresh output tensors in `names` order, the destination Data carrying the ABI ones)."""
    # an operator's outputs may not share storage with each other: every written leaf gets an allocation of its own and the native call
    # fills them through its `out=` path (the direct call carves its leaves from two slabs instead)
    tmpl = _template(m)
    qpos = leaves[_QPOS]
    batch = tuple(qpos.shape[:-1])
    outs, otop, ocon = [], {}, {}
    for n in names:
        ref = _leaf_of(tmpl, n)
        t = torch.empty(batch + tuple(ref.shape), dtype=qpos.dtype if n not in _INT_DTYPE else _INT_DTYPE[n], device=qpos.device)
        outs.append(t)
        if n in native.DATA_PATH:
            path = native.DATA_PATH[n]
            (ocon if len(path) == 2 else otop)[path[-1]] = t
    for n in _NAMES:  # the destination container carries the written leaves only (an expanded, stride-0 input leaf is not a valid destination)
        path = native.DATA_PATH[n]
        (ocon if len(path) == 2 else otop).setdefault(path[-1], None)
    return outs, d.replace(contact=d.contact.replace(**ocon), **otop)


def _checked_model(model_key, struct_uid, op, what):
    m = _model(model_key)
    if m._struct_uid != struct_uid:
        raise RuntimeError(f"mujoco_torch_amd::{op}: the Model handed to the traced {what} has another structure than the one it was traced with "
                           f"(different XML / cone / disabled constraints): trace a {what} of its own for it")
    return m


@torch.library.custom_op("mujoco_torch_amd::step_leaves", mutates_args=())
def step_leaves(leaves: list[torch.Tensor], model_key: torch.Tensor, struct_uid: str, fixed_iterations: bool, do_step: bool, stages: int) -> list[torch.Tensor]:
    from .forward import _run_native

    m = _checked_model(model_key, struct_uid, "step_leaves", "step")
    d = _data_of_leaves(m, leaves)
    outs, dout = _destination(m, d, leaves, out_names(m, do_step, stages))
    _run_native(m, d, fixed_iterations, do_step, dout, stages)
    return outs


@step_leaves.register_fake
def _(leaves, model_key, struct_uid, fixed_iterations, do_step, stages):
    m = _structure(struct_uid)
    tmpl = _template(m)
    qpos = leaves[_QPOS]
    batch = tuple(qpos.shape[:-1])
    outs = []
    for n in out_names(m, do_step, stages):
        ref = native.data_field_tensor(tmpl, n)
        dt = qpos.dtype if _NAMES.index(n) < _NREAL else _INT_DTYPE[n]
        outs.append(qpos.new_empty(batch + tuple(ref.shape), dtype=dt))
    return outs


def _step_leaves_vmap(info, in_dims, leaves, model_key, struct_uid, fixed_iterations, do_step, stages):
    B = info.batch_size
    moved = []
    for t, bd in zip(leaves, in_dims[0]):
        moved.append(t.unsqueeze(0).expand(B, *t.shape) if bd is None else t.movedim(bd, 0))
    outs = step_leaves(moved, model_key, struct_uid, fixed_iterations, do_step, stages)
    return outs, [0] * len(outs)


torch.library.register_vmap(step_leaves, _step_leaves_vmap)


@torch.library.custom_op("mujoco_torch_amd::inverse_leaves", mutates_args=())
def inverse_leaves(leaves: list[torch.Tensor], model_key: torch.Tensor, struct_uid: str) -> list[torch.Tensor]:
    from .forward import _run_native

    m = _checked_model(model_key, struct_uid, "inverse_leaves", "inverse")
    d = _data_of_leaves(m, leaves)
    outs, dout = _destination(m, d, leaves, inverse_out_names(m))
    _run_native(m, d, False, False, dout, 0x1F, inverse=True, qfrc_inverse=outs[-1])
    return outs


@inverse_leaves.register_fake
def _(leaves, model_key, struct_uid):
    m = _structure(struct_uid)
    tmpl = _template(m)
    qpos = leaves[_QPOS]
    batch = tuple(qpos.shape[:-1])
    return [qpos.new_empty(batch + tuple(_leaf_of(tmpl, n).shape), dtype=_INT_DTYPE.get(n, qpos.dtype)) for n in inverse_out_names(m)]


def _inverse_leaves_vmap(info, in_dims, leaves, model_key, struct_uid):
    B = info.batch_size
    moved = [t.unsqueeze(0).expand(B, *t.shape) if bd is None else t.movedim(bd, 0) for t, bd in zip(leaves, in_dims[0])]
    outs = inverse_leaves(moved, model_key, struct_uid)
    return outs, [0] * len(outs)


torch.library.register_vmap(inverse_leaves, _inverse_leaves_vmap)

_ABSENT = torch.empty(0)


def _leaves_of(d):
    con = d.contact
    leaves = []
    for n in _NAMES:
        path = native.DATA_PATH[n]
        t = getattr(con if len(path) == 2 else d, path[-1], None)
        leaves.append(t if isinstance(t, torch.Tensor) else _ABSENT)
    for n in _XNAMES:
        t = getattr(d, n, None)
        leaves.append(t if isinstance(t, torch.Tensor) else _ABSENT)
    return leaves


def _result(d, names, outs):
    con = d.contact
    top, cn = {}, {}
    for i in range(len(names)):
        if names[i] not in native.DATA_PATH:  # qfrc_inverse
            top[names[i]] = outs[i]
            continue
        path = native.DATA_PATH[names[i]]
        if len(path) == 2:
            cn[path[-1]] = outs[i]
        else:
            top[path[-1]] = outs[i]
    if cn:
        top["contact"] = con.replace(**cn)
    return d.replace(**top)


def run_through_op(m, d, fixed_iterations: bool, do_step: bool, stages: int):
    """``_run`` for calls that are being traced or vmapped: Dynamo-traceable Python around one operator call."""
    outs = torch.ops.mujoco_torch_amd.step_leaves(_leaves_of(d), m._op_key_t, m._struct_uid, fixed_iterations, do_step, stages)
    return _result(d, out_names(m, do_step, stages), outs)


def run_inverse_through_op(m, d):
    """``inverse`` under tracing / vmap: one ``inverse_leaves`` call."""
    outs = torch.ops.mujoco_torch_amd.inverse_leaves(_leaves_of(d), m._op_key_t, m._struct_uid)
    return _result(d, inverse_out_names(m), outs)


# ---- ray casting (ray.py): its own operator over the two geom-frame leaves and the rays ----------------------------------------

@torch.library.custom_op("mujoco_torch_amd::ray_leaves", mutates_args=())
def ray_leaves(geom_xpos: torch.Tensor, geom_xmat: torch.Tensor, pnt: torch.Tensor, vec: torch.Tensor, model_key: torch.Tensor, struct_uid: str,
               geomgroup: list[int], flg_static: bool, bodyexclude: list[int]) -> tuple[torch.Tensor, torch.Tensor]:
    from .ray import ray_native

    m = _checked_model(model_key, struct_uid, "ray_leaves", "ray")
    return ray_native(m, geom_xpos, geom_xmat, pnt, vec, (flg_static, bodyexclude, geomgroup))


@ray_leaves.register_fake
def _(geom_xpos, geom_xmat, pnt, vec, model_key, struct_uid, geomgroup, flg_static, bodyexclude):
    from .ray import check_args, filter_key

    filter_key(_structure(struct_uid).tables.ray, geomgroup, flg_static, bodyexclude)
    shape = check_args(geom_xpos, geom_xmat, pnt, vec)[0]
    return geom_xpos.new_empty(shape), geom_xpos.new_empty(shape, dtype=torch.int64)


def _ray_leaves_vmap(info, in_dims, geom_xpos, geom_xmat, pnt, vec, model_key, struct_uid, geomgroup, flg_static, bodyexclude):
    # the mapped dimension becomes the leading batch dimension of the Data; an unmapped frame leaf is broadcast, an unmapped ray keeps its
    # meaning: (3,) stays shared, anything else is the same for every mapped environment
    B = info.batch_size
    args = []
    for i, t in enumerate((geom_xpos, geom_xmat, pnt, vec)):
        bd = in_dims[i]
        if bd is not None:
            args.append(t.movedim(bd, 0))
        elif i >= 2 and t.dim() == 1:
            args.append(t)
        else:
            args.append(t.unsqueeze(0).expand(B, *t.shape))
    dist, geomid = ray_leaves(*args, model_key, struct_uid, geomgroup, flg_static, bodyexclude)
    return (dist, geomid), (0, 0)


torch.library.register_vmap(ray_leaves, _ray_leaves_vmap)


# ---- rendering (render.py): its own operator over the six pose leaves ------------------------------------------------------------

@torch.library.custom_op("mujoco_torch_amd::render_leaves", mutates_args=())
def render_leaves(geom_xpos: torch.Tensor, geom_xmat: torch.Tensor, cam_xpos: torch.Tensor, cam_xmat: torch.Tensor, light_xpos: torch.Tensor,
                  light_xdir: torch.Tensor, model_key: torch.Tensor, struct_uid: str, camera_id: int, width: int, height: int, shading: bool,
                  background: list[float], shadows: bool, fog: list[float], ssaa: int, u8: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    from .render import render_native

    m = _checked_model(model_key, struct_uid, "render_leaves", "render")
    opts = (camera_id, width, height, shading, tuple(background), shadows, tuple(fog), ssaa)
    return render_native(m, (geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir), opts, u8)


@render_leaves.register_fake
def _(geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir, model_key, struct_uid, camera_id, width, height, shading, background, shadows,
      fog, ssaa, u8):
    from .render import check_args, rgb_dtype

    m = _structure(struct_uid)
    batch = check_args(m, (geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir))
    opts = (camera_id, width, height, shading, tuple(background), shadows, tuple(fog), ssaa)
    return (geom_xpos.new_empty(batch + (height, width, 3), dtype=rgb_dtype(m, geom_xpos.dtype, opts, u8)),
            geom_xpos.new_empty(batch + (height, width)), geom_xpos.new_empty(batch + (height, width), dtype=torch.int64))


def _render_leaves_vmap(info, in_dims, geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir, model_key, struct_uid, *opts):
    # the mapped dimension becomes the leading batch dimension of the Data; an unmapped leaf is the same for every mapped environment
    B = info.batch_size
    args = [t.movedim(bd, 0) if bd is not None else t.unsqueeze(0).expand(B, *t.shape)
            for t, bd in zip((geom_xpos, geom_xmat, cam_xpos, cam_xmat, light_xpos, light_xdir), in_dims[:6])]
    return render_leaves(*args, model_key, struct_uid, *opts), (0, 0, 0)


torch.library.register_vmap(render_leaves, _render_leaves_vmap)


# ---- the support functions (support.py): one operator for the five ops, over the leaves each reads and its queries ---------------

@torch.library.custom_op("mujoco_torch_amd::support_leaves", mutates_args=())
def support_leaves(op: int, leaves: list[torch.Tensor], queries: list[torch.Tensor], model_key: torch.Tensor, struct_uid: str, body_ids: list[int],
                   listed: bool) -> list[torch.Tensor]:
    from .support import support_native

    m = _checked_model(model_key, struct_uid, "support_leaves", "support function")
    return support_native(m, op, leaves, queries, tuple(body_ids), listed)


@support_leaves.register_fake
def _(op, leaves, queries, model_key, struct_uid, body_ids, listed):
    from .support import plan

    return [leaves[0].new_empty(s) for s in plan(op, leaves, queries, tuple(body_ids), listed)[3]]


def _support_leaves_vmap(info, in_dims, op, leaves, queries, model_key, struct_uid, body_ids, listed):
    # the mapped dimension becomes the leading batch dimension of the Data; an unmapped leaf is broadcast, an unmapped query keeps its meaning:
    # a 1-D one stays shared, anything else is the same for every mapped environment
    B = info.batch_size
    lv = [t.movedim(bd, 0) if bd is not None else t.unsqueeze(0).expand(B, *t.shape) for t, bd in zip(leaves, in_dims[1])]
    qs = [t.movedim(bd, 0) if bd is not None else (t if t.dim() == 1 else t.unsqueeze(0).expand(B, *t.shape)) for t, bd in zip(queries, in_dims[2])]
    outs = support_leaves(op, lv, qs, model_key, struct_uid, body_ids, listed)
    return outs, [0] * len(outs)


torch.library.register_vmap(support_leaves, _support_leaves_vmap)
