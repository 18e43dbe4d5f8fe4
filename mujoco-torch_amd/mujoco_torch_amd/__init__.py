"""MI355X-native batched physics stepper behind the ``mujoco_torch.step`` API.

Drop-in for the hot path of vmoens/mujoco-torch (``mujoco_torch/__init__.py:41-136``):
``step``, ``forward``, ``inverse``, ``transition_fd``, ``inverse_fd``, ``transition_vjp``, ``differentiable_step``, ``tangent_pull``, ``tangent_push``, ``ray``, ``ray_geom``, ``render``, ``render_batch``, ``precompute_render_data``,
``rne_postconstraint``, ``subtree_vel``, ``fwd_postconstraint``, ``contact_force``, ``sensor_postconstraint``, ``energy``, ``energy_pos``, ``energy_vel``, ``geom_distance``, ``integrate_pos``, ``differentiate_pos``, ``normalize_quat``, ``state_sub``, ``state_add``, ``ik_site``, ``mul_jac_vec``, ``mul_jac_t_vec``, ``constraint_update``, ``efc_ar``, ``solve_pgs``, ``solve_noslip``, ``solve``, ``kinematics``, ``com_pos``, ``crb``, ``tendon_armature``, ``factor_m``, ``com_vel``, ``rne``, ``tendon``, ``transmission``, ``passive``, ``fwd_velocity``, ``fwd_actuation``, ``fwd_acceleration``, ``deriv_smooth_vel``, ``implicit``, ``euler``, ``jac``, ``jac_body``, ``jac_body_com``, ``jac_site``, ``jac_geom``, ``jac_subtree_com``, ``jac_dot``, ``angmom_mat``, ``apply_ft``, ``xfrc_accumulate``, ``mul_m``, ``solve_m``, ``full_m``, ``device_put``, ``make_data`` and the ``Model`` / ``Data`` / ``Contact`` /
``Option`` schema.  Use as ``import mujoco_torch_amd as mujoco_torch``.
"""

from . import mjcf  # noqa: F401
from ._enums import (  # noqa: F401
    BiasType,
    CamLightType,
    ConeType,
    ConstraintType,
    DisableBit,
    DynType,
    EnableBit,
    EqType,
    GainType,
    GeomType,
    IntegratorType,
    JacobianType,
    JointType,
    ObjType,
    SensorType,
    SolverType,
    TrnType,
    WrapType,
)
from .container import MjTensorClass, UnbatchedTensor  # noqa: F401
from .device import device_get_into, device_put  # noqa: F401
from .contact_sensors import contact_force, sensor_postconstraint  # noqa: F401
from .energy import energy, energy_pos, energy_vel  # noqa: F401
from .integrate import deriv_smooth_vel, euler, implicit  # noqa: F401
from .forward import forward, inverse, reset_where, step  # noqa: F401
from .geom_distance import geom_distance  # noqa: F401
from .qpos import differentiate_pos, integrate_pos, normalize_quat, state_add, state_sub  # noqa: F401
from .ik import IKResult, ik_site  # noqa: F401
from .constraint_space import ConstraintUpdate, EfcDual, constraint_update, efc_ar, mul_jac_t_vec, mul_jac_vec  # noqa: F401
from .pgs import PGSResult, solve_pgs  # noqa: F401
from .noslip import NoslipResult, solve_noslip  # noqa: F401
from .solver import SolveStats, solve  # noqa: F401
from .smooth import com_pos, com_vel, crb, factor_m, kinematics, rne, tendon_armature  # noqa: F401
from .dynamics import fwd_acceleration, fwd_actuation, fwd_velocity, passive, tendon, transmission  # noqa: F401
from .derivative import differentiable_step, inverse_fd, tangent_pull, tangent_push, transition_fd, transition_vjp  # noqa: F401
from .io import make_data  # noqa: F401
from .jacobian import angmom_mat, jac_body, jac_body_com, jac_dot, jac_geom, jac_site, jac_subtree_com  # noqa: F401
from .postconstraint import fwd_postconstraint, rne_postconstraint, subtree_vel  # noqa: F401
from .ray import ray, ray_geom  # noqa: F401
from .render import precompute_render_data, render, render_batch  # noqa: F401
from .support import apply_ft, full_m, jac, mul_m, solve_m, xfrc_accumulate  # noqa: F401
from .types import Contact, Data, Model, Option, Statistic  # noqa: F401

__version__ = "0.2.0"


def test_data_path(name: str = "") -> str:
    """Path of a bundled model file (``mujoco_torch_amd/test_data/``: the reference's ``mujoco_torch/test_data`` models plus
    the scenes of BASELINE.json's configs), e.g. ``test_data_path("humanoid.xml")``."""
    import os

    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_data", name)
