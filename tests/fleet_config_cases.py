"""Robot classes for the heterogeneous-fleet tests (tests/test_fleet_configs.py, tests/test_gpu_fleet_configs.py): class sets over the
fleets of tests/fleet_cases.py, a configuration per class and a class per scene (include/teb_amd.h: teb_amd_set_scene_configs).

  points : three classes over fleet_cases.point_fleet - the TebConfig defaults; a faster robot with a circular footprint, legacy
           obstacle association, an obstacle cost exponent and no inflation band; a holonomic robot with the shortest-path and the
           velocity-obstacle-ratio terms and the exact arc length. Every footprint is point-like: the fleet runs the point-like path.
  mixed  : four classes over fleet_cases.mixed_fleet(102) - a car-like forklift with a polygon footprint, a tugger with a line footprint
           that ignores via-points and weighs the path length instead of the time, a two-circles robot, a point diff-drive robot.
  sides  : two classes over fleet_cases.point_fleet - the defaults without obstacle weight (no dynamic-obstacle edges, the static
           obstacle terms weigh nothing) and the defaults without the weights of the velocity bounds (no velocity edges). They take
           the two sides of the kernel's conditions that no class of the two sets above takes.

Between them the classes take both sides of EVERY condition of csrc/teb_device.hpp (TEB_PF_EXPR_*) that reads the configuration:
SIDES lists them as functions of a TebConfig, tests/test_fleet_configs.py checks that both values occur.

The scenes whose bands sensitivity.band_tolerances (CPU oracle, analytic against numeric Jacobians, run with the scene's CLASS
configuration) marks ill-conditioned at attempt 0 are replaced by a later attempt of their own generator, as tests/fleet_cases.py does:
POINTS_REPLACED, MIXED_REPLACED; the sides set needs none (SIDES_REPLACED is empty): every class set runs against the oracle in full."""
import copy

import fleet_cases
from teb_local_planner_amd.config import RobotFootprintModel, TebConfig

POINTS_SEED, MIXED_SEED = 101, 102
POINTS_CLASS_OF = [0, 1, 2, 1, 0, 2]
MIXED_CLASS_OF = [0, 1, 2, 3, 0, 1]     # classes 0 and 1 hold two scenes each, classes 2 and 3 one
POINTS_REPLACED = {3: 4}
MIXED_REPLACED = {0: 5, 1: 3, 2: 3, 3: 3}
SIDES_CLASS_OF = [0, 1, 0, 1, 0, 1]
SIDES_REPLACED = {}

# the conditions of teb_device.hpp that read the configuration (the scene's and the launch's parts left out)
SIDES = {
    "EXACT_ARC": lambda c: bool(c.trajectory.exact_arc_length),
    "COST_EXPONENT": lambda c: c.optim.obstacle_cost_exponent != 1.0 and c.obstacles.min_obstacle_dist > 0.0,
    "NEW_ASSOCIATION": lambda c: not c.obstacles.legacy_obstacle_association,
    "VIA_POINTS": lambda c: c.optim.weight_viapoint != 0,
    "NONHOLONOMIC_VELOCITY": lambda c: c.robot.max_vel_y == 0,
    "ACCELERATION_EDGES": lambda c: not (c.optim.weight_acc_lim_x == 0 and c.optim.weight_acc_lim_theta == 0),
    "NONHOLONOMIC_ACCELERATION": lambda c: c.robot.max_vel_y == 0 or c.robot.acc_lim_y == 0,
    "TIME_OPTIMAL": lambda c: c.optim.weight_optimaltime != 0,
    "SHORTEST_PATH": lambda c: c.optim.weight_shortest_path != 0,
    "VELOCITY_OBSTACLE_RATIO": lambda c: c.optim.weight_velocity_obstacle_ratio > 0,
    "INFLATED": lambda c: c.obstacles.inflation_dist > c.obstacles.min_obstacle_dist,
    "DIVERGENCE_DETECTION": lambda c: bool(c.recovery.divergence_detection_enable),
    "KIN_DIFF_DRIVE": lambda c: c.robot.min_turning_radius == 0 or c.optim.weight_kinematics_turning_radius == 0,
    "KIN_EDGES": lambda c: not (c.optim.weight_kinematics_nh == 0 and c.optim.weight_kinematics_forward_drive == 0),
    "VELOCITY_EDGES": lambda c: not (c.optim.weight_max_vel_x == 0 and c.optim.weight_max_vel_theta == 0),
    "DYNAMIC_EDGES": lambda c: c.obstacles.include_dynamic_obstacles and c.optim.weight_obstacle != 0,
}
# the field groups in which the classes of a set differ from one another (what a launch that read ONE configuration would get wrong)
GROUPS = {
    "kinematics": lambda c: (c.robot.max_vel_y, c.robot.min_turning_radius, c.optim.weight_kinematics_nh),
    "velocity limits": lambda c: (c.robot.max_vel_x, c.robot.max_vel_theta, c.robot.acc_lim_x, c.robot.acc_lim_theta),
    "min_obstacle_dist": lambda c: (c.obstacles.min_obstacle_dist, c.obstacles.inflation_dist),
    "weights": lambda c: (c.optim.weight_max_vel_x, c.optim.weight_optimaltime, c.optim.weight_obstacle, c.optim.weight_shortest_path),
    "footprint": lambda c: (c.robot_model.type, c.robot_model.radius, tuple(c.robot_model.vertices)),
    "resize": lambda c: (c.trajectory.dt_ref, c.trajectory.dt_hysteresis),
    "selection": lambda c: (c.hcp.selection_cost_hysteresis, c.hcp.selection_prefer_initial_plan),
}


def _base(dynamic=True):
    c = TebConfig()
    c.obstacles.include_dynamic_obstacles = dynamic
    return c


def point_classes(dynamic=True):
    """[defaults, fast circular robot, holonomic robot]"""
    d = _base(dynamic)
    f = _base(dynamic)
    f.robot_model = RobotFootprintModel.circular(0.2)
    f.robot.max_vel_x, f.robot.max_vel_x_backwards, f.robot.max_vel_theta = 0.8, 0.3, 0.6
    f.robot.acc_lim_x, f.robot.acc_lim_theta = 0.8, 0.9
    f.optim.weight_max_vel_x, f.optim.weight_max_vel_theta, f.optim.weight_optimaltime = 3.0, 2.0, 2.0
    f.optim.weight_acc_lim_x, f.optim.weight_acc_lim_theta = 0.0, 0.0
    f.trajectory.dt_ref, f.trajectory.dt_hysteresis = 0.2, 0.05
    f.obstacles.min_obstacle_dist, f.obstacles.inflation_dist = 0.4, 0.3
    f.obstacles.legacy_obstacle_association, f.obstacles.obstacle_poses_affected = True, 15
    f.optim.obstacle_cost_exponent = 2.0
    f.recovery.divergence_detection_enable, f.recovery.divergence_detection_max_chi_squared = True, 5.0
    f.hcp.selection_cost_hysteresis, f.hcp.selection_prefer_initial_plan = 0.6, 0.7
    o = _base(dynamic)
    o.robot.max_vel_y, o.robot.acc_lim_y, o.robot.max_vel_x = 0.3, 0.4, 0.5
    o.optim.weight_max_vel_y, o.optim.weight_acc_lim_y = 2.0, 1.0
    o.optim.weight_kinematics_nh, o.optim.weight_kinematics_forward_drive = 0.0, 0.0
    o.optim.weight_shortest_path, o.optim.weight_velocity_obstacle_ratio = 0.5, 0.5
    o.trajectory.exact_arc_length = True
    o.obstacles.min_obstacle_dist, o.obstacles.inflation_dist = 0.3, 0.5
    o.hcp.selection_cost_hysteresis, o.hcp.selection_prefer_initial_plan = 0.9, 0.5
    return [d, f, o]


def mixed_classes(dynamic=True):
    """[car-like polygon forklift, line tugger, two-circles robot, point diff-drive robot]"""
    fork = _base(dynamic)
    fork.robot_model = RobotFootprintModel.polygon([(-0.2, -0.15), (0.4, -0.15), (0.4, 0.15), (-0.2, 0.15)])
    fork.robot.min_turning_radius, fork.optim.weight_kinematics_turning_radius = 0.4, 1.0
    fork.robot.max_vel_x, fork.robot.max_vel_theta = 0.5, 0.4
    fork.obstacles.min_obstacle_dist, fork.obstacles.inflation_dist = 0.3, 0.5
    tug = _base(dynamic)
    tug.robot_model = RobotFootprintModel.line((-0.2, 0.0), (0.4, 0.0))
    tug.optim.weight_viapoint = 0.0
    tug.optim.weight_optimaltime, tug.optim.weight_shortest_path = 0.0, 1.0
    tug.trajectory.dt_ref, tug.trajectory.dt_hysteresis = 0.35, 0.1
    tug.obstacles.min_obstacle_dist, tug.obstacles.inflation_dist = 0.35, 0.35
    tug.hcp.selection_cost_hysteresis, tug.hcp.selection_prefer_initial_plan = 0.7, 0.8
    two = _base(dynamic)
    two.robot_model = RobotFootprintModel.two_circles(0.3, 0.2, 0.15, 0.25)
    two.robot.max_vel_x, two.robot.acc_lim_x, two.robot.acc_lim_theta = 0.6, 0.7, 0.6
    two.optim.weight_max_vel_x, two.optim.weight_obstacle = 3.0, 40.0
    two.obstacles.min_obstacle_dist, two.obstacles.inflation_dist = 0.25, 0.45
    pt = _base(dynamic)
    pt.robot.max_vel_theta, pt.optim.weight_optimaltime = 0.5, 1.5
    pt.trajectory.dt_ref, pt.trajectory.dt_hysteresis = 0.25, 0.08
    return [fork, tug, two, pt]


def side_classes(dynamic=True):
    """[defaults without obstacle weight, defaults without the weights of the velocity bounds]"""
    free = _base(dynamic)
    free.optim.weight_obstacle = 0.0
    unbounded = _base(dynamic)
    unbounded.optim.weight_max_vel_x, unbounded.optim.weight_max_vel_theta = 0.0, 0.0
    return [free, unbounded]


class ClassedFleet:
    """fleet: a fleet_cases.Fleet (its cfg is the HANDLE's configuration, which a launch with the map must ignore); cfgs: the classes;
    class_of [n_scenes]"""

    def __init__(self, fleet, cfgs, class_of):
        assert len(class_of) == fleet.n_scenes and max(class_of) < len(cfgs)
        self.fleet, self.cfgs, self.class_of = fleet, cfgs, [int(k) for k in class_of]

    def cfg_of_scene(self, s):
        return self.cfgs[self.class_of[s]]

    def cfg_of_band(self, b):
        return self.cfg_of_scene(int(self.fleet.scene_of[b]))

    def scenes_of_class(self, k):
        return [s for s in range(self.fleet.n_scenes) if self.class_of[s] == k]


def classed_point_fleet(stride=96, polygon_class=None):
    """polygon_class: that class gets a polygon footprint - the whole fleet then runs the generic distance path"""
    f = fleet_cases.point_fleet(POINTS_SEED, stride=stride, replaced=POINTS_REPLACED)
    cfgs = point_classes()
    if polygon_class is not None:
        cfgs[polygon_class].robot_model = RobotFootprintModel.polygon([(-0.15, -0.1), (0.25, -0.1), (0.25, 0.1), (-0.15, 0.1)])
    return ClassedFleet(f, cfgs, POINTS_CLASS_OF)


def classed_mixed_fleet(stride=96):
    f = fleet_cases.mixed_fleet(MIXED_SEED, stride=stride, replaced=MIXED_REPLACED)
    return ClassedFleet(f, mixed_classes(), MIXED_CLASS_OF)


def classed_sides_fleet(stride=96):
    f = fleet_cases.point_fleet(POINTS_SEED, stride=stride, replaced=SIDES_REPLACED)
    return ClassedFleet(f, side_classes(), SIDES_CLASS_OF)


CLASSED_FLEETS = {"points": classed_point_fleet, "mixed": classed_mixed_fleet, "sides": classed_sides_fleet}


def growing_classed_fleet():
    """tests/test_gpu_fleet.py's _growing_fleet with classes: every class keeps the default resize parameters except class 1, whose
    dt_ref = 0.1 splits every interval of its bands - only ITS bands outgrow the optimistic blocks-in-LDS layout of a 400-pose handle."""
    f = fleet_cases.point_fleet(103, stride=400, poses=100, obstacles=(20, 60), spacing=0.08, amplitude=0.3)
    cfgs = [_base(), _base()]
    cfgs[1].trajectory.dt_ref, cfgs[1].trajectory.dt_hysteresis = 0.1, 0.02
    return ClassedFleet(f, cfgs, [0, 1, 0, 0, 1, 0])


def handle_config_that_differs(cfgs):
    """A handle configuration that no class equals in the fields a fleet launch, the consumers and the selection read: a launch that
    read it instead of the class table would be found out."""
    c = copy.deepcopy(cfgs[0])
    c.robot.max_vel_x, c.robot.max_vel_y = 0.27, 0.11
    c.obstacles.min_obstacle_dist = 0.45
    c.trajectory.dt_ref = 0.31
    c.hcp.selection_cost_hysteresis, c.hcp.selection_prefer_initial_plan = 1.0, 1.0
    c.robot_model = RobotFootprintModel.point()
    return c


def as_bytes(cfg):
    return bytes(cfg.to_c())

