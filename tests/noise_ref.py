"""numpy restatement of the fluctuation term of the MLAPM scenario frame (piml_amd/csrc/noise.hpp, piml_noise_force,
piml_scenario_step_mlapm_noise) for the tests: the draws from tests/philox_ref.philox4x32_10 and the float32 recursion.
Everything but z is bit-exact float32; z is double arithmetic rounded once, so a device z may differ from this one by
one float32 ulp where the two `log` / `cos` differ in the last double bit."""
import math

import numpy as np

from philox_ref import philox4x32_10

NOISE_STREAM = 0x5CE40000
F32 = np.float32
TWO_M24 = 5.9604644775390625e-8


def law(An, noise_tau, dt):
    """(rho, amp) as float32: float64 arithmetic rounded once (ops_scenario.noise_law)"""
    rho = math.exp(-dt / noise_tau) if noise_tau > 0 else 0.0
    return F32(rho), F32(An * math.sqrt(1.0 - rho * rho))


def normal(wa, wb):
    u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * TWO_M24
    u2 = (wb >> np.uint64(8)).astype(np.float64) * TWO_M24
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(F32)


def draws(seed, frame, slots):
    """z (len(slots), 2) float32 of (seed, frame) for the slots given"""
    seed, frame = int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame)
    slots = np.asarray(slots, np.uint64)
    w = philox4x32_10(np.full(slots.shape, frame & 0xFFFFFFFF, np.uint64), np.full(slots.shape, frame >> 32, np.uint64), slots,
                      np.full(slots.shape, NOISE_STREAM | 1, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    w = [np.asarray(x, np.uint64) for x in w]
    return np.stack((normal(w[0], w[1]), normal(w[2], w[3])), -1)


def step(eta, rho, amp, z):
    """rho eta + amp z, every operation a float32 one rounded on its own"""
    eta, z = np.asarray(eta, F32), np.asarray(z, F32)
    return ((F32(rho) * eta).astype(F32) + (F32(amp) * z).astype(F32)).astype(F32)


def force(eta, seeds, frame, rho, amp, present=None, z=None):
    """piml_noise_force on eta (members, N, 2): (eta_out, z); rows with present == 0 keep eta and get z = 0.  z: the normals to
    use instead of the restatement's own (the device's, for a bitwise check of the recursion)"""
    eta = np.asarray(eta, F32)
    members, N = eta.shape[:2]
    if z is None:
        z = np.stack([draws(seeds[m], frame, np.arange(N)) for m in range(members)])
    out = step(eta, rho, amp, z)
    if present is not None:
        keep = np.asarray(present) != 0
        out = np.where(keep[..., None], out, eta)
        z = np.where(keep[..., None], z, F32(0))
    return out, z
