"""Chosen operands for every simulation modifier (the macro ops M_AGE_TICK ... of hnb_vm.h) and an independent reference of what each must give.

Data and numpy only, like tests/math_lattice.py, whose binary32 definitions this module reuses (`ref_vec3`: dot = (x x' + y y') + z z',
normalize(v) = v * (1 / length(v)), cross; `ref_ieee`: step, sign, min, max, mix, smoothstep, abs). Every formula is the WGSL text the reference
emits for the modifier, one numpy binary32 operation per WGSL operation:

  age / reap     src/lib.rs:1223-1262        age = age + dt; is_alive = age < lifetime
  Euler          src/lib.rs:1106-1120        position += velocity * dt (appended after the modifiers)
  Accel          accel.rs:79-86              velocity += (accel) * dt                      (the product is a rounding of its own)
  RadialAccel    accel.rs:174-182            radial = normalize(position - origin); velocity += radial * ((accel) * dt)
  TangentAccel   accel.rs:289-299            tangent = normalize(cross(axis, radial)); velocity += tangent * ((accel) * dt)
  LinearDrag     force.rs:284-297            velocity *= max(0, 1 - drag * dt)
  Conform        force.rs:196-230            with the early return when surface_dist > influence_dist (false for a NaN distance)
  KillSphere     kill.rs:76-96               dot(d, d) < or > sqr_radius
  KillAabb       kill.rs:156-181             any(abs(d) > half) or all(abs(d) < half); a NaN never kills
  VelocitySphere velocity.rs:131-137         velocity = normalize(position - center) * speed
  PositionCircle position.rs:71-99           PositionSphere position.rs:168-201     PositionCone3d position.rs:283-315  (these draw: vfx_common.wgsl:266-343)
  VelocityCircle velocity.rs:57-70           VelocityTangent velocity.rs:200-213    (with Cone3d: the emitter transform, init context only)

A table is a short stack of modifiers with P parameter rows and Q particle rows (position, velocity, age, lifetime); the tests run every
parameter row against every particle row (P * Q rows). Several small tables per modifier, each built around the operands where that modifier
can go wrong, not one cross product: a lattice taken over wholesale is NaN nearly everywhere and proves little.

The transcendental builtins inside the drawing shapes - sqrt, pow(., 1/3), cos, sin, acos - are NOT restated here: `ref_update` takes them
through the `builtins` argument (the tests pass oracle.math1 / math2 element by element). Their accuracy is tests/math_lattice.py's business;
what is pinned here is the composition around them.

Not reachable, so not in a table: LinearDrag's `1 - drag * dt` = -0 (a round-to-nearest difference of 1 and a product is never -0).
"""
import numpy as np

import math_lattice as ml
from math_lattice import INF, f32, ref_ieee, ref_vec3, step_ulps, u32

DT = f32(1.0 / 60.0)
SUB1, SUB2, SUB3 = (u32(k).view(f32) for k in (1, 2, 3))             # one, two, three subnormal units
T75, T74 = f32(2.0 ** -75), f32(2.0 ** -74)                            # T75^2 rounds to 0 (1 / length = inf), T74^2 is subnormal
BIG_CENTRE = (1024.5, -2048.25, 4096.125)                             # pos - centre rounds for offsets below 2^-13 ... 2^-11
_Q = dict(all="ignore")


def V(*rows):
    with np.errstate(**_Q):
        return np.array(rows, np.float64).astype(f32).reshape(len(rows), -1)


def S(*vals):
    with np.errstate(**_Q):
        return np.array(vals, np.float64).astype(f32)


# ---- the draws (vfx_common.wgsl:266-343), uint32 arithmetic ----------------------------------------------------------------------------
def pcg_hash(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    state = (x * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return (((word >> 22) ^ word) & 0xFFFFFFFF).astype(u32)


def to_float01(u):
    """bitcast<f32>((u & 0x007fffff) | 0x3f800000) - 1"""
    return ((np.asarray(u, u32) & u32(0x007FFFFF)) | u32(0x3F800000)).view(f32) - f32(1.0)


def frand(seed):
    """seed = pcg_hash(seed); return to_float01(pcg_hash(seed)): (new seed, value)"""
    seed = pcg_hash(seed)
    return seed, to_float01(pcg_hash(seed))


def update_seed(index, frame_seed):
    """vfx_update.wgsl:138: seed = pcg_hash(particle_index ^ spawner.seed)"""
    return pcg_hash(np.asarray(index, u32) ^ u32(frame_seed & 0xFFFFFFFF))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
TAU = f32(6.283185307179586)


def _col(s):
    return np.asarray(s, f32)[:, None]


def _normalize(v):
    return ref_vec3("normalize", v)


def _dot(a, b):
    return ref_vec3("dot", a, b)


def ref_accel(pos, vel, dt, accel):
    return vel + accel * dt


def ref_drag(pos, vel, dt, drag):
    return vel * _col(ref_ieee("max", np.zeros_like(drag), f32(1.0) - drag * dt))


def ref_radial(pos, vel, dt, origin, accel):
    return vel + _normalize(pos - origin) * _col(accel * dt)


def ref_tangent(pos, vel, dt, origin, axis, accel):
    radial = _normalize(pos - origin)
    tangent = _normalize(ref_vec3("cross", axis, radial))
    return vel + tangent * _col(accel * dt)


def ref_vel_sphere(pos, vel, dt, center, speed):
    return _normalize(pos - center) * _col(speed)


def ref_conform(pos, vel, dt, origin, radius, influence, accel, max_speed, shell, sticky):
    rel_pos = origin - pos
    origin_dist = ref_vec3("length", rel_pos)
    origin_dir = _normalize(rel_pos)
    surface_dist = origin_dist - radius
    returned = surface_dist > influence
    cur_radial_speed = _dot(vel, origin_dir)
    shell_factor = ref_ieee("smoothstep", np.zeros_like(shell), shell, ref_ieee("abs", surface_dist))
    max_radial_speed = ref_ieee("sign", surface_dist) * shell_factor * max_speed
    delta_speed = max_radial_speed - cur_radial_speed
    sticky_accel = accel * sticky
    conforming_accel = ref_ieee("mix", sticky_accel, accel, shell_factor)
    conforming_delta_speed = dt * conforming_accel
    k = ref_ieee("sign", delta_speed) * ref_ieee("min", ref_ieee("abs", delta_speed), conforming_delta_speed)
    return np.where(returned[:, None], vel, vel + _col(k) * origin_dir).astype(f32)


def ref_kill_sphere(pos, center, sqr_radius, inside):
    d = pos - center
    sqr = _dot(d, d)
    return np.where(inside, sqr < sqr_radius, sqr > sqr_radius)


def ref_kill_aabb(pos, center, half, inside):
    dist = np.abs(pos - center)
    return np.where(inside, (dist < half).all(axis=1), (dist > half).any(axis=1))


def ref_pos_circle(seed, builtins, center, axis, radius, volume):
    """position.rs:71-99. builtins: {"sqrt", "cos", "sin", ...: f32 -> f32, element by element}"""
    n = axis
    sign = ref_ieee("step", np.zeros_like(n[:, 2]), n[:, 2]) * f32(2.0) - f32(1.0)
    a = f32(-1.0) / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    tangent = np.stack([f32(1.0) + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], axis=1)
    bitangent = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], axis=1)
    if volume:
        seed, u = frand(seed)
        r = builtins["sqrt"](u) * radius
    else:
        r = radius
    seed, u = frand(seed)
    theta = u * TAU
    direction = tangent * _col(builtins["cos"](theta)) + bitangent * _col(builtins["sin"](theta))
    return seed, (center + _col(r) * direction).astype(f32)


def ref_pos_sphere(seed, builtins, center, radius, volume):
    """position.rs:168-201"""
    if volume:
        seed, u = frand(seed)
        r = builtins["cbrt"](u) * radius
    else:
        r = radius
    seed, u = frand(seed)
    theta = u * TAU
    seed, u = frand(seed)
    z = u * f32(2.0) - f32(1.0)
    sinphi = builtins["sin"](builtins["acos"](z))
    x = sinphi * builtins["cos"](theta)
    y = sinphi * builtins["sin"](theta)
    return seed, (center + _col(r) * np.stack([x, y, z], axis=1)).astype(f32)


# ---- tables --------------------------------------------------------------------------------------------------------------------------
# the parameters of each modifier kind, in the order of its constructor: (name, components)
KINDS = {
    "accel": (("accel", 3),),
    "drag": (("drag", 1),),
    "radial": (("origin", 3), ("accel", 1)),
    "tangent": (("origin", 3), ("axis", 3), ("accel", 1)),
    "vel_sphere": (("center", 3), ("speed", 1)),
    "conform": (("origin", 3), ("radius", 1), ("influence", 1), ("accel", 1), ("max_speed", 1), ("shell", 1), ("sticky", 1)),
    "kill_sphere": (("center", 3), ("sqr_radius", 1)),
    "kill_aabb": (("center", 3), ("half", 3)),
    "pos_circle": (("center", 3), ("axis", 3), ("radius", 1)),
    "pos_sphere": (("center", 3), ("radius", 1)),
}
CONFORM_DEFAULTS = {"shell": 0.1, "sticky": 2.0}     # force.rs:190-194: the literals written when the modifier has no expression for them


class Op:
    """one modifier of a stack. params: {name: (P, components) array}; flags: kill_inside, volume, defaults (conform parameters left to the reference's literal)"""

    def __init__(self, kind, inside=False, volume=False, defaults=(), **params):
        self.kind, self.inside, self.volume, self.defaults = kind, inside, volume, tuple(defaults)
        self.params = {}
        for name, comps in KINDS[kind]:
            if name in self.defaults:
                continue
            p = np.asarray(params.pop(name), f32)
            self.params[name] = p.reshape(len(p), comps)
        assert not params, params

    def mnemonic(self):
        return {"accel": "M_VEL_ADD", "drag": "M_VEL_SCALE", "radial": "M_RADIAL_ACCEL", "tangent": "M_TANGENT_ACCEL", "vel_sphere": "M_VEL_SPHERE",
                "conform": "M_CONFORM_SPHERE", "kill_sphere": "M_KILL_SPHERE", "kill_aabb": "M_KILL_AABB", "pos_circle": "M_POS_CIRCLE",
                "pos_sphere": "M_POS_SPHERE"}[self.kind]


class Table:
    """ops: the stack; particles: {"pos", "vel": (Q, 3), "age", "lifetime": (Q,)}; every parameter array has P rows. `edges`: {edge kind: mask over
    the P * Q rows}; `nan_is_the_point`: the edge kinds whose result is NaN by design. Row r of the run is parameter row r // Q, particle r % Q."""

    def __init__(self, name, ops, pos, vel=None, age=None, lifetime=None, dt=DT, edges=None, nan_is_the_point=(), has_age=True, streamable=True, seed=0x5EED):
        self.name, self.ops, self.dt, self.has_age, self.streamable, self.seed = name, ops, f32(dt), has_age, streamable, seed
        self.pos = np.asarray(pos, f32)
        self.Q = len(self.pos)
        self.vel = np.zeros((self.Q, 3), f32) if vel is None else np.asarray(vel, f32)
        self.age = np.zeros(self.Q, f32) if age is None else np.asarray(age, f32)
        self.lifetime = np.full(self.Q, 1e9, f32) if lifetime is None else np.asarray(lifetime, f32)
        ps = {len(p) for op in ops for p in op.params.values()}
        assert len(ps) <= 1, (name, ps)
        self.P = ps.pop() if ps else 1
        self.n = self.P * self.Q
        self.edges_fn, self.nan_is_the_point, self.no_motion = edges or (lambda t: {}), tuple(nan_is_the_point), False

    # the P * Q rows
    def particle(self, what):
        return np.tile(getattr(self, what), (self.P,) + (1,) * (getattr(self, what).ndim - 1))

    def param(self, op, name):
        """(n, components), or (n,) for a scalar"""
        if name in op.defaults:
            return np.full(self.n, CONFORM_DEFAULTS[name], f32)
        p = np.repeat(op.params[name], self.Q, axis=0)
        return p if p.shape[1] == 3 else p[:, 0]

    def edges(self):
        return self.edges_fn(self)

    def prow(self):
        return np.repeat(np.arange(self.P), self.Q)

    def qrow(self):
        return np.tile(np.arange(self.Q), self.P)


def ref_update(t, builtins=None, index=None):
    """One update frame of table t over its P * Q rows: {"pos", "vel", "age", "alive"}. index: the particle index of every row (the drawing shapes)."""
    with np.errstate(**_Q):
        pos, vel, age, life = t.particle("pos"), t.particle("vel"), t.particle("age"), t.particle("lifetime")
        alive = np.ones(t.n, bool)
        if t.has_age:
            age = age + t.dt
            alive = age < life
        seed = None if index is None else update_seed(index, t.seed)
        for op in t.ops:
            a = [t.param(op, name) for name, _ in KINDS[op.kind]]
            if op.kind == "accel": vel = ref_accel(pos, vel, t.dt, *a)
            elif op.kind == "drag": vel = ref_drag(pos, vel, t.dt, *a)
            elif op.kind == "radial": vel = ref_radial(pos, vel, t.dt, *a)
            elif op.kind == "tangent": vel = ref_tangent(pos, vel, t.dt, *a)
            elif op.kind == "vel_sphere": vel = ref_vel_sphere(pos, vel, t.dt, *a)
            elif op.kind == "conform": vel = ref_conform(pos, vel, t.dt, *a)
            elif op.kind == "kill_sphere": alive = alive & ~ref_kill_sphere(pos, *a, op.inside)
            elif op.kind == "kill_aabb": alive = alive & ~ref_kill_aabb(pos, *a, op.inside)
            elif op.kind == "pos_circle": seed, pos = ref_pos_circle(seed, builtins, *a, op.volume)
            elif op.kind == "pos_sphere": seed, pos = ref_pos_sphere(seed, builtins, *a, op.volume)
            else: raise KeyError(op.kind)
        pos = pos + vel * t.dt
        return {"pos": pos.astype(f32), "vel": vel.astype(f32), "age": age.astype(f32), "alive": alive}


# ---- operand design ------------------------------------------------------------------------------------------------------------------
def _around(x):
    return [float(step_ulps(f32(x), -1)), float(f32(x)), float(step_ulps(f32(x), 1))]


def _params(base, *variants):
    """parameter rows: `base` with one or a few entries replaced per variant -> {name: array}"""
    rows = [dict(base, **v) for v in variants]
    return {k: np.array([np.atleast_1d(np.asarray(r[k], np.float64)) for r in rows]).astype(f32) for k in base}


# separations (position - centre) of the normalising modifiers
SEPARATIONS = V((0, 0, 0),                                   # 0: at the centre: 0 * inf = NaN
                (float(SUB1),) * 3, (float(T75), -float(T75), float(T75)),   # 1, 2: the squared length rounds to 0: 1 / length = inf
                (float(T74), float(T74), 0.5 * float(T74)),   # 3: a subnormal squared length
                (2e19, 2e19, -2e19),                          # 4: the squared length overflows: 1 / length = 0
                (0, 5, 0),                                    # 5: along (0, 1, 0): parallel to the axis of the tangent tables
                (1, 2, 3), (-0.3, 0.1, 7.5), (1.0 / 3.0, -2.0 / 3.0, 1e-3), (1e-20, 1e20, 1.0), (3, 4, 0), (-2, 0, 0), (0, 0, -0.25), (7, -7, 7))
SEP_VEL = V((0, 0, 0), (1, -2, 0.5), (0, 0, 0), (1e-3, 0, 0), (1, 1, 1), (0, 0, 0), (0, 0, 0), (1, -2, 0.5), (-1, 0, 0), (0, 3, 0), (0.5, 0.5, 0.5), (0, 0, 0), (1, 2, 3), (0, -1, 0))


def _sep_edges(t):
    q = t.qrow()
    return {"particle at the centre": q == 0, "reciprocal of the length is inf": (q == 1) | (q == 2), "subnormal squared length": q == 3,
            "squared length overflows": q == 4}


def _with_centres(sep, centres):
    """particles placed at centre + separation for each centre: the positions, and the centre of each"""
    with np.errstate(**_Q):
        return np.concatenate([f32(c) + sep for c in np.asarray(centres, f32)])


def radial_table():
    p = _params(dict(origin=(0, 0, 0), accel=2.0), {}, dict(accel=-0.5), dict(accel=0.0), dict(accel=np.inf), dict(accel=float(SUB3)), dict(origin=(1, 2, 3)),
                dict(origin=(1, 2, 3), accel=-7.0), dict(origin=BIG_CENTRE), dict(origin=(np.nan, 0, 0)))
    pos = np.concatenate([SEPARATIONS, V((1, 2, 3), (1 + 2.0 ** -20, 2, 3), (4, 6, 3)), V(BIG_CENTRE) + V((2.0 ** -12, 0.25, -1))])
    vel = np.concatenate([SEP_VEL, V((0, 0, 0), (0, 0, 0), (1, 1, 1), (0, 0, 0))])

    def edges(t):
        e = _sep_edges(t)
        e["NaN centre"] = t.prow() == 8
        return e
    return Table("radial", [Op("radial", **p)], pos, vel, edges=edges, nan_is_the_point=("particle at the centre", "NaN centre"))


AXES = dict(unit=(0, 1, 0), zero=(0, 0, 0), long=(0, 2, 0), nan=(0, np.nan, 0), skew=(0, 0.6, 0.8), neg=(-0.0, -1, -0.0))


def tangent_table():
    base = dict(origin=(0, 0, 0), axis=AXES["unit"], accel=3.0)
    p = _params(base, {}, dict(axis=AXES["long"]), dict(axis=AXES["skew"]), dict(axis=AXES["neg"]), dict(axis=AXES["zero"]), dict(axis=AXES["nan"]), dict(accel=-1.0),
                dict(accel=0.0), dict(origin=(1, 2, 3), axis=AXES["skew"]), dict(origin=BIG_CENTRE, axis=(1, 0, 0)))
    pos = np.concatenate([SEPARATIONS, V((1, 2, 3)) + V((2, 0, 0), (0, 0.6, 0.8)), V(BIG_CENTRE) + V((2.0 ** -12, 0.25, -1))])
    vel = np.concatenate([SEP_VEL, V((0, 0, 0), (1, 1, 1), (0, 0, 0))])

    def edges(t):
        e, pr, q = _sep_edges(t), t.prow(), t.qrow()
        e.update({"axis parallel to the radius": ((pr == 0) | (pr == 1) | (pr == 3)) & (q == 5), "zero axis": pr == 4, "non-unit axis": pr == 1, "NaN axis": pr == 5})
        return e
    return Table("tangent", [Op("tangent", **p)], pos, vel, edges=edges,
                 nan_is_the_point=("particle at the centre", "axis parallel to the radius", "zero axis", "NaN axis", "reciprocal of the length is inf", "squared length overflows"))


def vel_sphere_table():
    p = _params(dict(center=(0, 0, 0), speed=3.0), {}, dict(speed=0.0), dict(speed=-1.0), dict(speed=np.inf), dict(speed=float(SUB2)), dict(center=(1, 2, 3)),
                dict(center=BIG_CENTRE, speed=0.5), dict(center=(0, np.inf, 0)))
    pos = np.concatenate([SEPARATIONS, V((1, 2, 3), (4, 6, 3)), V(BIG_CENTRE) + V((2.0 ** -12, 0.25, -1))])
    vel = np.concatenate([SEP_VEL, V((0, 0, 0), (1, 1, 1), (0, 0, 0))])
    return Table("vel_sphere", [Op("vel_sphere", **p)], pos, vel, edges=_sep_edges, nan_is_the_point=("particle at the centre",), streamable=False)


def conform_tables():
    """positions with an exact distance from the centre: |(3, 4, 0)| = 5, |(6, 8, 0)| = 10, |(0.75, 0, 1)| = 1.25"""
    acc = 6.0
    at = float(f32(DT * f32(acc)))                                                   # dt * attraction_accel: the conforming delta speed where shell_factor = 1
    base = dict(origin=(0, 0, 0), radius=2.0, influence=30.0, accel=acc, max_speed=1.5, shell=0.5, sticky=2.0)
    lo, mid, hi = _around(3.0)
    vs = [{}, dict(influence=mid), dict(influence=lo), dict(influence=hi),              # 1-3: surface_dist = 3 at, above and below the influence distance
          dict(radius=5.0), dict(radius=5.0, shell=0.0),                                # 4, 5: on the surface: sign(0) = 0; with shell 0: smoothstep(0, 0, 0)
          dict(shell=0.0), dict(shell=-0.5), dict(shell=4.0), dict(sticky=0.0), dict(sticky=-1.0, shell=4.0),   # 6-10
          dict(max_speed=at), dict(max_speed=_around(at)[0]), dict(max_speed=_around(at)[2]), dict(max_speed=np.inf), dict(max_speed=0.0),   # 11-15
          dict(accel=0.0), dict(accel=np.inf, shell=0.0), dict(radius=np.inf), dict(influence=np.inf), dict(influence=np.nan), dict(origin=(1, 2, 3), radius=1.0),   # 16-21
          dict(origin=BIG_CENTRE, radius=0.0), dict(radius=-1.0)]
    p = _params(base, *vs)
    pos = V((3, 4, 0), (3, 4, 0), (6, 8, 0), (0.75, 0, 1), (0, 0, 0), (float(T75), 0, 0), (2e19, 2e19, -2e19), (1, 2, 3), (4, 6, 3), (0, -2, 0), (0.3, 0.4, 0), (-3, 0, -4))
    vel = V((0, 0, 0), (1, -2, 0.5), (0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, 1), (-1, -1, 0), (0, 5, 0), (0, 0, 0), (0.1, 0.2, 0.3))

    def edges(t):
        pr, q = t.prow(), t.qrow()
        exact = (q == 0) | (q == 1) | (q == 11)
        return {"surface distance at the influence distance": (pr == 1) & exact, "one ulp inside the influence distance": (pr == 3) & exact,
                "one ulp outside the influence distance": (pr == 2) & exact, "on the surface": (pr == 4) & exact, "shell 0": (pr == 6) | (pr == 5), "negative shell": pr == 7,
                "sticky 0": pr == 9, "delta_speed at conforming_delta_speed": (pr == 11) & (q == 0), "delta_speed one ulp below": (pr == 12) & (q == 0),
                "delta_speed one ulp above": (pr == 13) & (q == 0), "infinite maximum speed": pr == 14, "particle at the centre": q == 4,
                "NaN influence distance": pr == 20}
    nanpt = ("particle at the centre",)
    out = [Table("conform", [Op("conform", **p)], pos, vel, edges=edges, nan_is_the_point=nanpt)]
    # the reference's own literals for shell (0.1) and sticky (2.0), dt 0 and a negative dt
    few = {k: v[[0, 1, 4, 11, 14]] for k, v in p.items() if k not in ("shell", "sticky")}
    out.append(Table("conform_defaults", [Op("conform", defaults=("shell", "sticky"), **few)], pos, vel, edges=lambda t: {"default shell and sticky": np.ones(t.n, bool)}))
    some = {k: v[[0, 1, 4, 6, 9, 11, 14]] for k, v in p.items()}
    out.append(Table("conform_dt0", [Op("conform", **some)], pos, vel, dt=0.0, edges=lambda t: {"dt 0": np.ones(t.n, bool)}))
    out.append(Table("conform_dtneg", [Op("conform", **some)], pos, vel, dt=-1.0 / 120.0, edges=lambda t: {"negative dt": np.ones(t.n, bool)}))
    return out


def kill_sphere_tables():
    off = V((3, 4, 0), (3, 4, 2.0 ** -11), (3, float(step_ulps(f32(4.0), -1)), 0), (0, 0, 0), (float(T75), 0, 0), (float(T74), 0, 0), (1e20, 0, 0), (1, 2, 2), (5, 0, 0),
            (float(step_ulps(f32(5.0), 1)), 0, 0), (0, float(step_ulps(f32(5.0), -1)), 0), (0, 0, -6), (0.5, 0.5, 0.5), (float(SUB1), 0, 0), (0, np.nan, 0))
    centres = V((0, 0, 0), BIG_CENTRE)
    pos = _with_centres(off, centres)
    r2 = _around(25.0) + [0.0, -0.0, float(SUB1), np.inf, np.nan, 0.75]
    rows = [dict(center=c, sqr_radius=r) for c in centres.tolist() for r in r2]
    p = _params(dict(center=(0, 0, 0), sqr_radius=25.0), *rows)

    def edges(t):
        pr, q = t.prow() % len(r2), t.qrow() % len(off)
        own = (t.prow() // len(r2)) == (t.qrow() // len(off))       # the particle sits around this row's centre
        return {"on the surface": own & (pr == 1) & np.isin(q, (0, 8)), "one ulp inside": own & (((pr == 2) & np.isin(q, (0, 8))) | ((pr == 1) & (q == 10))),
                "one ulp outside": own & (((pr == 0) & np.isin(q, (0, 8))) | ((pr == 1) & (q == 9))), "at the centre": own & (q == 3), "squared radius 0": pr == 3, "squared radius -0": pr == 4,
                "subnormal squared radius": pr == 5, "infinite squared radius": pr == 6, "NaN squared radius": pr == 7, "large centre": t.prow() >= len(r2),
                "subnormal squared distance": q == 5, "NaN position": q == 14}
    return [Table(f"kill_sphere_{'inside' if inside else 'outside'}", [Op("kill_sphere", inside=inside, **p)], pos, edges=edges, nan_is_the_point=("NaN position",))
            for inside in (False, True)]


def kill_aabb_tables():
    h = (1.0, 2.0, 3.0)
    off = [(0, 0, 0), (-1, -2, -3), (0.5, 1, 1.5), (5, 5, 5), (0.5, -5, 0), (float(SUB1), 0, 0), (float(SUB2), 0, 0), (float(SUB3), 0, 0), (0.5, np.nan, 0), (0.5, 1, np.inf)]
    for axis in range(3):                                              # on the surface and one ulp either side, per axis and per sign
        for v in _around(h[axis]):
            for s in (1.0, -1.0):
                o = [0.25, 0.25, 0.25]
                o[axis] = s * v
                off.append(tuple(o))
    off = V(*off)
    centres = V((0, 0, 0), BIG_CENTRE)
    pos = _with_centres(off, centres)
    halves = [h, (1, 0, 3), (1, np.inf, 3), (1, np.nan, 3), (float(SUB2), 2, 3), (np.inf, np.inf, np.inf), (0.25, 0.25, 0.25), (-1, 2, 3)]
    rows = [dict(center=c, half=hh) for c in centres.tolist() for hh in halves]
    p = _params(dict(center=(0, 0, 0), half=h), *rows)

    def edges(t):
        pr, q = t.prow() % len(halves), t.qrow() % len(off)
        surf = (q >= 10) & ((t.prow() // len(halves)) == (t.qrow() // len(off)))       # around this row's centre
        k = (q - 10) // 2 % 3                                          # 0: one ulp inside, 1: on the surface, 2: one ulp outside
        return {"on the surface": (pr == 0) & surf & (k == 1), "one ulp inside": (pr == 0) & surf & (k == 0), "one ulp outside": (pr == 0) & surf & (k == 2),
                "half size with a 0": pr == 1, "half size with an inf": pr == 2, "half size with a NaN": pr == 3, "infinite half size": pr == 5,
                "subnormal half size against subnormal differences": (pr == 4) & np.isin(q, (5, 6, 7)), "large centre": t.prow() >= len(halves), "NaN position": q == 8}
    return [Table(f"kill_aabb_{'inside' if inside else 'outside'}", [Op("kill_aabb", inside=inside, **p)], pos, edges=edges, nan_is_the_point=("NaN position",))
            for inside in (False, True)]


# ---- the component-wise stacks: AgeEuler, Accel, Drag, DragAccel, AccelDrag ----------------------------------------------------------------
FMA_X = float(f32(1.0 + 2.0 ** -12))            # x * x rounds (1 + 2^-11 + 2^-24 -> 1 + 2^-11); x * x - (1 + 2^-11) is 2^-24 fused and 0 in two roundings


def _one_component(values, rest):
    """every value in x only, in y only, in z only, the other two components `rest`"""
    rows = []
    for v in values:
        for axis in range(3):
            r = [rest, rest, rest]
            r[axis] = v
            rows.append(tuple(r))
    return V(*rows)


_CW_EDGES = [0.0, -0.0, float(SUB1), -float(SUB3), float(ml.FLT_MAX), -float(ml.FLT_MAX), np.inf, -np.inf, np.nan, FMA_X, 1e-30, -2.5]


def componentwise_tables():
    """The flat path of the streaming kernel picks the component of a vec3 operand by a rotation: every edge sits in ONE of x, y, z, so that a
    wrong rotation moves it. dt = 1/60, and once dt = 4 where `v * dt` overflows although a fused `pos + v * dt` would not; and dt = x = 1 + 2^-12
    against v = x, pos = -(1 + 2^-11), where the fused form keeps the 2^-24 that the rounded product loses."""
    vel = np.concatenate([_one_component(_CW_EDGES, 0.75), V((1, -2, 0.5), (-(1 + 2.0 ** -11),) * 3, (1e38, -1e38, 1e38), (FMA_X, FMA_X, FMA_X))])
    pos = np.concatenate([np.tile(V((1, 2, 3), (-0.5, 0, 1e10), (0, 0, 0)), (len(_CW_EDGES), 1)), V((0, 0, 0), (0, 0, 0), (-3e38, 3e38, -3e38), (-(1 + 2.0 ** -11),) * 3)])
    Q = len(vel)
    age = np.linspace(0.0, 2.0, Q).astype(f32)
    life = np.where(np.arange(Q) % 5 == 4, 1.0, 5.0).astype(f32)
    accels = dict(accel=V((0, -9.81, 0), (np.nan, 0, 0), (0, 0, np.inf), (3, 0, 0), (0, float(SUB2), 0), (1e38, 0, 0), (0, 0, -3e38), (FMA_X, FMA_X, FMA_X), (-0.0, 0.0, -0.0)))
    P = len(accels["accel"])
    # (row for row beside the accelerations: the drags whose factor is 0 stand beside a finite acceleration, where 0 * velocity is not NaN)
    drags = dict(drag=S(60.0, 0.0, 0.5, 120.0, np.inf, -np.inf, -2.0, np.nan, float(SUB1))[:P])

    def edges(t):
        q = t.qrow()
        e = {"edge in x only": (q < 3 * len(_CW_EDGES)) & (q % 3 == 0), "edge in y only": (q < 3 * len(_CW_EDGES)) & (q % 3 == 1), "edge in z only": (q < 3 * len(_CW_EDGES)) & (q % 3 == 2)}
        if t.dt == f32(4.0):
            e["v * dt overflows, the fused sum would not"] = q == Q - 2
        if t.dt == f32(FMA_X):
            e["fused and unfused differ in the last bit"] = (q == Q - 1) | (q == Q - 3)
        for op in t.ops:
            if op.kind == "drag":
                d = t.param(op, "drag")
                with np.errstate(**_Q):
                    x = f32(1.0) - d * t.dt
                e.update({"1 - drag * dt negative": np.isfinite(d) & (x < 0), "NaN drag": np.isnan(d), "infinite drag": d == INF})
                if (x == 0).any():
                    e["1 - drag * dt = 0"] = x == 0
        return e
    stacks = {"age_euler": [], "accel": ["accel"], "drag": ["drag"], "drag_accel": ["drag", "accel"], "accel_drag": ["accel", "drag"]}
    out = []
    for name, kinds in stacks.items():
        for tag, dt in (("", DT), ("_dt4", 4.0), ("_dtfma", FMA_X)):
            ops = [Op(k, **(accels if k == "accel" else drags)) for k in kinds]
            out.append(Table(name + tag, ops, pos, vel, age, life, dt=dt, edges=edges))
    return out


def age_table():
    """ProgAge: one AGE_TICK and nothing else (a position that nothing moves, no velocity)"""
    age, life = ml.cross(S(0.0, -0.0, -1e-3, float(SUB1), 0.5, 1.0, float(step_ulps(f32(1.0) - DT, -1)), float(f32(1.0) - DT), float(step_ulps(f32(1.0) - DT, 1)), 1e9),
                         S(0.0, -1.0, float(SUB1), 0.5, 1.0, float(ml.FLT_MAX), np.inf, float(f32(0.5) + DT), float(step_ulps(f32(0.5) + DT, 1))))
    t = Table("age", [], np.zeros((len(age), 3), f32), None, age, life, edges=lambda t: {"age + dt at the lifetime": (t.age + DT) == t.lifetime})
    t.no_motion = True
    return t


def stack_tables():
    """the remaining pre-built sequences: Accel + KillAabb (activate.rs) and the force field's Conform, Conform, KillAabb, KillSphere"""
    pos = V((0, 0, 0), (1, 0, 0), (3, 4, 0), (0, 6, 0), (0, float(step_ulps(f32(6.0), 1)), 0), (-6, 0, 0), (0.25, 0.25, 7), (2, 2, 2), (-3, 0, -4), (0.75, 0, 1), (5.5, 5.5, 5.5), (0, 0, 0.2))
    vel = V((1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0), (0, -1, 0), (0.5, 0.5, 0.5), (0, 0, 0), (1, 2, 3), (0, 0, 0), (-1, 0, 0))
    a = _params(dict(accel=(0, -3, 0), center=(0, 0, 0), half=(6, 6, 6)), {}, dict(half=(6, np.inf, 6)), dict(center=(0.5, 0, 0), half=(0.5, 6, 6)), dict(accel=(0, 0, 1e38)),
                dict(half=(0, 0, 0)), dict(half=(3, 3, 3)))
    out = [Table("accel_kill_aabb", [Op("accel", accel=a["accel"]), Op("kill_aabb", center=a["center"], half=a["half"])], pos, vel)]
    base = dict(o1=(0, 0, 0), r1=2.0, i1=30.0, a1=6.0, m1=1.5, s1=0.5, k1=2.0, o2=(1, 2, 3), r2=1.0, i2=3.0, a2=-2.0, m2=0.5, s2=0.0, k2=0.0, bc=(0, 0, 0), bh=(6, 6, 6),
                sc=(0, 0, 0), sr=0.04)
    f = _params(base, {}, dict(i1=3.0), dict(r1=5.0, s1=0.0), dict(bh=(6, 6, np.inf), sr=0.0), dict(sr=np.nan, m1=np.inf), dict(sc=(3, 4, 0), sr=float(SUB1), i2=np.inf))
    ops = [Op("conform", origin=f["o1"], radius=f["r1"], influence=f["i1"], accel=f["a1"], max_speed=f["m1"], shell=f["s1"], sticky=f["k1"]),
           Op("conform", origin=f["o2"], radius=f["r2"], influence=f["i2"], accel=f["a2"], max_speed=f["m2"], shell=f["s2"], sticky=f["k2"]),
           Op("kill_aabb", center=f["bc"], half=f["bh"]), Op("kill_sphere", inside=True, center=f["sc"], sqr_radius=f["sr"])]
    out.append(Table("force_field", ops, pos, vel))
    return out


def shape_tables():
    """SetPositionCircle / SetPositionSphere in the UPDATE context (position.rs:113,215: Init | Update): they draw from pcg_hash(index ^ frame seed)"""
    axes = V((0, 0, 1), (0, 0, -1), (0, 0, -0.0), (1, 0, 0), (0, 0.6, 0.8), (0, 0, 0), (2, 0, 0), (0, 1, np.nan))
    radii = S(2.5, 0.0, -1.0, float(SUB3), np.inf)
    ia, ir = ml.cross(np.arange(len(axes)), np.arange(len(radii)))
    pc = dict(center=np.tile(V((1, 2, 3)), (len(ia), 1)), axis=axes[ia], radius=radii[ir])
    pos = np.tile(V((0, 0, 0), (1, 1, 1), (9, 9, 9), (0, -1, 0)), (2, 1))
    vel = np.tile(V((0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 2, 0)), (2, 1))

    def cedges(t):
        pa, pr = ia[t.prow()], ir[t.prow()]
        names = ("axis +z", "axis -z", "n.z = -0", "axis x", "axis (0, 0.6, 0.8)", "zero axis", "non-unit axis", "NaN axis z")
        e = {n: pa == k for k, n in enumerate(names)}
        e.update({"radius 0": pr == 1, "radius -1": pr == 2, "subnormal radius": pr == 3, "infinite radius": pr == 4})
        return e
    out = [Table(f"pos_circle_{'volume' if vol else 'surface'}", [Op("pos_circle", volume=vol, **pc)], pos, vel, edges=cedges, streamable=False,
                 nan_is_the_point=("NaN axis z",)) for vol in (False, True)]
    ps = _params(dict(center=(1, 2, 3), radius=2.5), {}, dict(radius=0.0), dict(radius=np.inf), dict(radius=-1.0), dict(radius=float(SUB3)), dict(center=BIG_CENTRE),
                 dict(center=(0, np.inf, 0)))

    def sedges(t):
        pr = t.prow()
        return {"radius 0": pr == 1, "infinite radius": pr == 2, "infinite centre": pr == 6}
    out += [Table(f"pos_sphere_{'volume' if vol else 'surface'}", [Op("pos_sphere", volume=vol, **ps)], np.tile(pos, (4, 1)), np.tile(vel, (4, 1)), edges=sedges, streamable=False)
            for vol in (False, True)]
    return out


CHUNK = 4096                       # slots per chunk of the streaming update (csrc/hnb_program.h kChunk)
BIG_CAPACITY = 2 * CHUNK + 300     # all alive: two whole chunks, which may take the flat path, and a partial one, which may not
BIG_STACKS = ("age_euler", "accel", "drag", "drag_accel", "accel_drag")


def big_table(name):
    """A component-wise table over BIG_CAPACITY particles: its Q lattice particles at slots 0.., across the seam 4095 | 4096 and in the partial chunk,
    ordinary particles (which stay alive and finite for many frames) everywhere else; three of the parameter rows."""
    t = tables()[name]
    n, Q = BIG_CAPACITY, t.Q
    i = np.arange(n)
    pos = np.stack([i * 1e-3, np.ones(n), -(i % 7)], axis=1).astype(f32)
    vel = np.stack([0.1 + (i % 5) * 0.01, np.full(n, 0.2), np.full(n, -0.3)], axis=1).astype(f32)
    age, life = ((i % 11) * 0.01).astype(f32), (5.0 + (i % 3)).astype(f32)
    where = np.concatenate([np.arange(Q), CHUNK - Q // 2 + np.arange(Q), 2 * CHUNK + 10 + np.arange(Q)])
    for k, slot in enumerate(where):
        pos[slot], vel[slot], age[slot], life[slot] = t.pos[k % Q], t.vel[k % Q], t.age[k % Q], t.lifetime[k % Q]
    ops = [Op(op.kind, **{k: p[[0, 3, 7]] for k, p in op.params.items()}) for op in t.ops]
    big = Table(name + "_big", ops, pos, vel, age, life, dt=t.dt)
    big.lattice_slots = where
    return big


def cut(t, rows=384, params=None):
    """the table over its first particles only, so that it has about `rows` rows (the shared launches of small programs); params: the first parameter rows only"""
    ops = t.ops
    if params is not None:
        ops = []
        for op in t.ops:
            o = Op(op.kind, inside=op.inside, volume=op.volume, defaults=op.defaults, **{k: p[:params] for k, p in op.params.items()})
            ops.append(o)
    P = t.P if params is None else min(t.P, params)
    q = max(1, min(t.Q, rows // P))
    c = Table(t.name + "_cut", ops, t.pos[:q], t.vel[:q], t.age[:q], t.lifetime[:q], dt=t.dt, streamable=t.streamable, seed=t.seed)
    c.no_motion = t.no_motion
    return c


# ---- ages and lifetimes through the host's proofs ------------------------------------------------------------------------------------------
AGE_CAPACITY = 3 * CHUNK + 500
AGE_TICKS = (1.0 / 60.0, 0.0, 1e-6, -1.0 / 120.0, 1.0 / 60.0, 1.0 / 30.0, 1.0 / 60.0, 1.0 / 60.0, 0.0, 1.0 / 60.0, 1.0 / 120.0, 1.0 / 60.0)
AGE_RESPAWN = (7, 300)            # (frame, particles): frame 8 of the twelve spawns again


def age_lifetime_planes():
    """AGE and LIFETIME over AGE_CAPACITY slots: ordinary values everywhere (ages 0 .. 0.5 of lifetimes 0.55 .. 1.45: some die within the twelve frames),
    the edge pairs at slots 0.., across the seam 4095 | 4096 and in the partial chunk; chunk 2 is left ordinary. Returns (age, lifetime, edge slots)."""
    n = AGE_CAPACITY
    i = np.arange(n)
    age = ((i % 51) * 0.01).astype(f32)
    life = (0.55 + (i % 10) * 0.1).astype(f32)
    dt = DT
    one = f32(1.0)
    with np.errstate(**_Q):
        pairs = [(a, 1.0) for a in (-0.0, -1e-3, float(SUB1), np.nan, np.inf, float(step_ulps(one - dt, -1)), float(one - dt), float(step_ulps(one - dt, 1)))]
        pairs += [(0.25, l) for l in (0.0, -1.0, float(SUB1), float(ml.FLT_MAX), np.inf, np.nan, float(f32(0.25) + dt), float(step_ulps(f32(0.25) + dt, 1)))]
        pairs += [(np.nan, np.nan), (np.inf, np.inf), (-0.0, 0.0), (float(SUB1), float(SUB2)), (0.0, np.inf), (-1e-3, float(ml.FLT_MAX))]
    pairs = V(*pairs)
    K = len(pairs)
    where = np.concatenate([np.arange(K), CHUNK - K // 2 + np.arange(K), 3 * CHUNK + 20 + np.arange(K)])
    for k, slot in enumerate(where):
        age[slot], life[slot] = pairs[k % K]
    return age, life, where


def ref_alive_after_tick(age, lifetime, dt):
    """src/lib.rs:1236-1246: age = age + dt; is_alive = age < lifetime"""
    with np.errstate(**_Q):
        return (np.asarray(age, f32) + f32(dt)) < np.asarray(lifetime, f32)


# ---- the position and velocity modifiers in the INIT context ---------------------------------------------------------------------------------
def ref_xform_dir(xf, v):
    """transform * vec4(v, 0) (vfx_init.wgsl:157-164: the mat4x4 of the spawner's 3x4 rows): the columns times v.x, v.y, v.z, 0, summed left to right.
    xf: (n, 12) row-major 3x4. xf[3] * 0 is NaN for an infinite translation."""
    return np.stack([((xf[:, 4 * r] * v[:, 0] + xf[:, 4 * r + 1] * v[:, 1]) + xf[:, 4 * r + 2] * v[:, 2]) + xf[:, 4 * r + 3] * f32(0.0) for r in range(3)], axis=1).astype(f32)


def ref_pos_cone3d(seed, builtins, height, base_radius, top_radius, xf):
    """position.rs:283-315"""
    seed, u = frand(seed)
    alpha_h = builtins["cbrt"](u)
    h = height * alpha_h
    r0 = base_radius + (top_radius - base_radius) * alpha_h
    seed, u = frand(seed)
    r = r0 * builtins["sqrt"](u)
    seed, u = frand(seed)
    theta = u * TAU
    p = np.stack([r * builtins["cos"](theta), h, r * builtins["sin"](theta)], axis=1)
    return seed, ref_xform_dir(xf, p)


def ref_vel_circle(pos, center, axis, speed, xf):
    """velocity.rs:57-70"""
    delta = pos - center
    radial = _normalize(delta - _col(_dot(delta, axis)) * axis)
    return ref_xform_dir(xf, radial) * _col(speed)


def ref_vel_tangent(pos, origin, axis, speed, xf):
    """velocity.rs:200-213"""
    tangent = _normalize(ref_vec3("cross", axis, pos - origin))
    return ref_xform_dir(xf, tangent) * _col(speed)


IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
TRANSFORMS = V(IDENTITY, (0, -2, 0, 5, 2, 0, 0, -1, 0, 0, 0.5, 3), (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 0, np.inf, 0, 1, 0, 0, 0, 0, 1, 0),
               (1, 0, 0, 0, 0, np.inf, 0, 0, 0, 0, 1, 0))      # identity, rotation with scale and translation, a zero row, an infinite translation, an infinite scale
INIT_Q = 64


class InitTable:
    """An init stack - a position modifier, then a velocity modifier - with P parameter rows (one effect and one spawning frame of INIT_Q particles each;
    `xf`: the frame's emitter transform). pos / vel: (kind, {parameter: (P, components)}, volume)."""

    def __init__(self, name, pos, vel, xf, seed=0xBEE5, edges=None, nan_is_the_point=()):
        self.name, self.pos, self.vel, self.xf, self.seed, self.P, self.Q = name, pos, vel, np.asarray(xf, f32), seed, len(xf), INIT_Q
        self.n = self.P * self.Q
        self.row_edges, self.nan_is_the_point = edges or {}, tuple(nan_is_the_point)     # {edge kind: mask over the P parameter rows}

    def edges(self):
        """{edge kind: mask over the P * Q rows}"""
        return {k: np.repeat(np.asarray(m, bool), self.Q) for k, m in self.row_edges.items()}


INIT_KINDS = dict(KINDS, cone3d=(("height", 1), ("base_radius", 1), ("top_radius", 1)), vel_circle=(("center", 3), ("axis", 3), ("speed", 1)),
                  vel_tangent=(("origin", 3), ("axis", 3), ("speed", 1)))


def ref_init(t, builtins):
    """what the init stores right behind the two modifiers: {"pos", "vel"} over the P * Q rows (row = parameter row * Q + slot)"""
    with np.errstate(**_Q):
        rep = lambda p: (lambda a: a if a.shape[1] == 3 else a[:, 0])(np.repeat(np.asarray(p, f32).reshape(t.P, -1), t.Q, axis=0))
        xf = np.repeat(t.xf, t.Q, axis=0)
        seed = update_seed(np.tile(np.arange(t.Q), t.P), t.seed)          # (vfx_init.wgsl:154: the same derivation as the update's)
        kind, params, volume = t.pos
        a = [rep(params[name]) for name, _ in INIT_KINDS[kind]]
        if kind == "pos_sphere": seed, pos = ref_pos_sphere(seed, builtins, *a, volume)
        elif kind == "pos_circle": seed, pos = ref_pos_circle(seed, builtins, *a, volume)
        else: seed, pos = ref_pos_cone3d(seed, builtins, *a, xf)
        kind, params, _ = t.vel
        a = [rep(params[name]) for name, _ in INIT_KINDS[kind]]
        if kind == "vel_sphere": vel = ref_vel_sphere(pos, None, None, *a)
        elif kind == "vel_circle": vel = ref_vel_circle(pos, *a, xf)
        else: vel = ref_vel_tangent(pos, *a, xf)
        return {"pos": pos.astype(f32), "vel": vel.astype(f32)}


def init_tables():
    """{name: InitTable}: radius or height 0 and inf, top equal to base, the particle at the velocity's centre (radius 0), the circle's axes, the transforms"""
    nx = len(TRANSFORMS)
    out = []
    rows = [dict(center=(1, 2, 3), radius=2.5, c2=(1, 2, 3), speed=3.0), dict(center=(1, 2, 3), radius=0.0, c2=(1, 2, 3), speed=3.0),
            dict(center=(1, 2, 3), radius=np.inf, c2=(0, 0, 0), speed=1.0), dict(center=(0, 0, 0), radius=float(SUB3), c2=(0, 0, 0), speed=-2.0),
            dict(center=BIG_CENTRE, radius=2.0 ** -12, c2=BIG_CENTRE, speed=2.0), dict(center=(0, 0, 0), radius=1.0, c2=(0.5, 0, 0), speed=0.0),
            dict(center=(0, 0, 0), radius=1.0, c2=(0, 0, 0), speed=2.0), dict(center=(1, 2, 3), radius=0.5, c2=(0, 0, 0), speed=1.0),
            dict(center=(-1, 0, 4), radius=3.0, c2=(-1, 0, 4), speed=-1.0), dict(center=(0, 0, 0), radius=2.0, c2=(0, 1, 0), speed=0.25),
            dict(center=(0, 0, 0), radius=-1.0, c2=(0, 0, 0.5), speed=float(SUB3)), dict(center=(5, 5, 5), radius=1e-3, c2=(5, 5, 5), speed=np.inf)]
    p = _params(rows[0], *rows)
    k = np.arange(len(rows))
    e = {"radius 0: the particle at the velocity's centre": k == 1, "infinite radius": k == 2, "subnormal radius": k == 3, "negative radius": k == 10,
         "infinite speed": k == 11, "speed 0": k == 5, "large centre": k == 4}
    for vol in (False, True):
        out.append(InitTable(f"init_sphere_{'volume' if vol else 'surface'}", ("pos_sphere", dict(center=p["center"], radius=p["radius"]), vol),
                             ("vel_sphere", dict(center=p["c2"], speed=p["speed"]), False), np.tile(V(IDENTITY), (len(rows), 1)), edges=e,
                             nan_is_the_point=("radius 0: the particle at the velocity's centre", "infinite radius")))
    axes = V((0, 0, 1), (0, 0, -1), (0, 0, -0.0), (1, 0, 0), (0, 0.6, 0.8), (0, 0, 0), (2, 0, 0), (0, 1, np.nan))
    radii = S(2.5, 0.0, -1.0, float(SUB3), np.inf)
    ia, ir = ml.cross(np.arange(len(axes)), np.arange(len(radii)))
    ja, jr = ml.cross(np.array([0, 1, 2, 3, 4, 6]), np.array([0, 2, 0, 2, 0]))          # and as many rows again of the ordinary radii on the axes that have a basis,
    ia, ir = np.concatenate([ia, ja]), np.concatenate([ir, jr])                          # so that most of the table is not NaN
    P = len(ia)
    ix = np.array([0, 1, 2, 1, 0, 1, 0, 3, 0, 1, 0, 4])[np.arange(P) % 12]               # the transforms: mostly finite
    centre = np.tile(V((1, 2, 3)), (P, 1))
    names = ("axis +z", "axis -z", "n.z = -0", "axis x", "axis (0, 0.6, 0.8)", "zero axis", "non-unit axis", "NaN axis z")
    e = {n: ia == k for k, n in enumerate(names)}
    e.update({"radius 0": ir == 1, "radius -1": ir == 2, "subnormal radius": ir == 3, "infinite radius": ir == 4, "transform with a zero row": ix == 2,
              "transform with an infinite translation": ix == 3, "transform with an infinite scale": ix == 4})
    nanpt = ("NaN axis z", "radius 0", "subnormal radius", "infinite radius", "transform with an infinite translation")
    for vol in (False, True):
        out.append(InitTable(f"init_circle_{'volume' if vol else 'surface'}", ("pos_circle", dict(center=centre, axis=axes[ia], radius=radii[ir]), vol),
                             ("vel_circle", dict(center=centre, axis=axes[ia], speed=np.full((P, 1), 1.5, f32)), False), TRANSFORMS[ix], edges=e, nan_is_the_point=nanpt))
    cones = [dict(height=4.0, base_radius=2.0, top_radius=0.5), dict(height=0.0, base_radius=2.0, top_radius=0.5), dict(height=np.inf, base_radius=1.0, top_radius=1.0),
             dict(height=1.0, base_radius=1.5, top_radius=1.5), dict(height=1.0, base_radius=0.0, top_radius=0.0), dict(height=-1.0, base_radius=np.inf, top_radius=0.5)]
    tang = [dict(origin=(0, 0, 0), axis=(0, 1, 0), speed=1.5), dict(origin=(0, 0, 0), axis=(0, 0, 0), speed=1.5), dict(origin=(1, 2, 3), axis=(0, 2, 0), speed=-1.0),
            dict(origin=(0, 0, 0), axis=(0, np.nan, 0), speed=1.0), dict(origin=(0, 0, 0), axis=(0, 0.6, 0.8), speed=np.inf)]
    # (cone, tangent, transform): each varied alone from the ordinary row, a few pairs, and ordinary rows under the finite transforms
    trip = [(c, 0, 0) for c in range(len(cones))] + [(0, k, 0) for k in range(1, len(tang))] + [(0, 0, x) for x in range(1, nx)]
    trip += [(0, 2, 1), (3, 0, 1), (1, 2, 2), (3, 4, 1), (4, 2, 3), (0, 0, 1), (3, 2, 0), (4, 0, 1), (0, 2, 2), (3, 2, 1), (4, 2, 0), (1, 0, 1), (0, 2, 0), (3, 0, 2)]
    ic, it, ix = (np.array([r[k] for r in trip]) for k in range(3))
    pc, pt = _params(cones[0], *cones), _params(tang[0], *tang)
    e = {"height 0": ic == 1, "infinite height": ic == 2, "top equal to base": ic == 3, "radii 0": ic == 4, "infinite base radius": ic == 5, "zero axis": it == 1,
         "non-unit axis": it == 2, "NaN axis": it == 3, "infinite speed": it == 4, "transform with a zero row": ix == 2, "transform with an infinite translation": ix == 3,
         "transform with an infinite scale": ix == 4}
    out.append(InitTable("init_cone", ("cone3d", {k: v[ic] for k, v in pc.items()}, True), ("vel_tangent", {k: v[it] for k, v in pt.items()}, False), TRANSFORMS[ix], edges=e,
                         nan_is_the_point=("infinite height", "infinite base radius", "zero axis", "NaN axis", "transform with an infinite translation",
                                           "transform with an infinite scale")))     # (an infinite position component: 0 * inf in the cross product)
    return {t.name: t for t in out}


_TABLES = None


def tables():
    """{name: Table}, built once"""
    global _TABLES
    if _TABLES is None:
        ts = [radial_table(), tangent_table(), vel_sphere_table()] + conform_tables() + kill_sphere_tables() + kill_aabb_tables() + componentwise_tables()
        ts += [age_table()] + stack_tables() + shape_tables()
        _TABLES = {t.name: t for t in ts}
        assert len(_TABLES) == len(ts)
    return _TABLES


def prebuilt_sequence(t):
    """the name of the pre-built streaming kernel (csrc/hanabi_amd.hip) that the table's stack matches exactly, or None"""
    kinds = tuple(op.kind for op in t.ops)
    if t.no_motion:
        return "ProgAge" if not kinds else None
    return {(): "ProgAgeEuler", ("accel",): "ProgAccel", ("drag",): "ProgDrag", ("drag", "accel"): "ProgDragAccel", ("accel", "drag"): "ProgAccelDrag",
            ("accel", "kill_aabb"): "ProgAccelKillAabb", ("radial",): "ProgRadial", ("conform", "conform", "kill_aabb", "kill_sphere"): "ProgForceField"}.get(kinds)


KILL_TABLES = ("kill_sphere_outside", "kill_sphere_inside", "kill_aabb_outside", "kill_aabb_inside")
# the pre-built sequences of csrc/hanabi_amd.hip and the table that runs each, parameters as effect properties
AOT = {"ProgAge": "age", "ProgAgeEuler": "age_euler", "ProgAccel": "accel", "ProgDrag": "drag", "ProgDragAccel": "drag_accel", "ProgAccelDrag": "accel_drag",
       "ProgAccelKillAabb": "accel_kill_aabb", "ProgRadial": "radial", "ProgForceField": "force_field"}
