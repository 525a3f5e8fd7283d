"""Burst effects whose update is a streamable stack WITHOUT a pre-built kernel (hnb_program_kernel_info: update=jit-stream): what
tests/test_jit_fused_steps.py and tests/test_gpu_simulate_steps_jit.py run through hnb_simulate_steps. Every one is reaped by lifetime only
(uniform(2, 3) s), so the host can prove spans of list-free frames between the burst and the die-off."""
import bevy_hanabi_amd as bh

A = bh.Attribute
ZERO3, Z3 = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)


def _burst(cap, w, update, life=(2.0, 3.0)):
    init = [bh.SetPositionSphereModifier(w.lit(ZERO3).expr(), w.lit(4.0).expr(), bh.ShapeDimension.Surface),
            bh.SetAttributeModifier(A.VELOCITY, ((w.rand(bh.VectorType.VEC3F) * w.lit(2.0) - w.lit(1.0)) * w.lit(3.0)).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(life[0]).uniform(w.lit(life[1])).expr())]
    asset = bh.EffectAsset(cap, bh.SpawnerSettings.once(float(cap)), w.finish())
    for m in init:
        asset = asset.init(m)
    for m in update:
        asset = asset.update(m)
    return asset


def tangent_drag(cap, life=(2.0, 3.0)):
    """TangentAccel + LinearDrag: the update of the reference's portal example (the asset of tools/steps_ab.py --asset tangent_drag)."""
    w = bh.ExprWriter()
    return _burst(cap, w, [bh.TangentAccelModifier(w.lit(ZERO3).expr(), w.lit(Z3).expr(), w.lit(30.0).expr()), bh.LinearDragModifier(w.lit(2.0).expr())], life)


def accel_radial_tangent_drag(cap):
    w = bh.ExprWriter()
    return _burst(cap, w, [bh.AccelModifier(w.lit((0.0, -3.0, 0.0)).expr()),
                           bh.RadialAccelModifier(w.lit((0.5, 0.0, 0.0)).expr(), w.lit(-3.0).expr()),
                           bh.TangentAccelModifier(w.lit(ZERO3).expr(), w.lit(Z3).expr(), w.lit(30.0).expr()),
                           bh.LinearDragModifier(w.lit(2.0).expr())])


def pinned_set_accel(cap):
    """A SetAttributeModifier in the update whose value depends on `time` (HNB_OP_M_PIN_SET: every step's uniform block differs), then Accel."""
    w = bh.ExprWriter()
    t = w.time()
    return _burst(cap, w, [bh.SetAttributeModifier(A.VELOCITY, t.sin().vec3(t * w.lit(-2.0), t * t).expr()),
                           bh.AccelModifier(w.lit((0.0, -9.0, 0.0)).expr())])
