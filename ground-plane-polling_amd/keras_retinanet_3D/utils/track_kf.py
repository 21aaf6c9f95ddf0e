"""
The ground-plane Kalman filter of DESIGN.md section 4.34 in NumPy: the only place where its expressions are host code.  utils/track.py
(step_np) and utils/track_smooth.py (smooth_cells' forward pass) call these functions; csrc/track_kf.h is the device form,
tests/track_kf_oracle.py and tests/track_smooth_oracle.py are the loop-written oracles.  No GPU, no library and no BLAS: one NumPy
operation per float64 operation of the rule, in the rule's association -- the tests compare words with ==.  Arguments are floats or
float64 arrays over any leading shape; a covariance P is a sequence of the ten words Axx Axz Azz Bxx Bxz Bzx Bzz Cxx Cxz Czz, a noise R
the three words Rxx Rxz Rzz.  Nothing is changed in place; the caller sets np.errstate.
"""
import numpy as np

PI = float(np.pi)
TWO_PI = 2.0 * PI


def wrap(a):
    """ into [-pi, pi): the wrap of csrc/track_kf.h, operation for operation """
    a = a - TWO_PI * np.floor(a / TWO_PI)
    a = np.where(a < 0.0, a + TWO_PI, a)
    a = np.where(a >= TWO_PI, a - TWO_PI, a)
    return np.where(a >= PI, a - TWO_PI, a)


def row_noise(x, z, noise):
    """ "row noise" of a row at (x, z) -> the array (3, ...) Rxx Rxz Rzz: sigma radial0 + radial1 rho along the viewing ray on the ground
    plane, tangential0 + tangential1 rho across it; noise: utils.track.check_noise's dict """
    (r0, r1), (t0, t1) = noise['radial'], noise['tangential']
    rho = np.sqrt((x * x) + (z * z))
    far = rho != 0.0
    ux, uz = np.where(far, x / rho, 0.0), np.where(far, z / rho, 1.0)
    sr, st = r0 + (r1 * rho), t0 + (t1 * rho)
    vr, vt = sr * sr, st * st
    dv = vr - vt
    return np.stack([vt + (dv * (ux * ux)), dv * (ux * uz), vt + (dv * (uz * uz))])


def born_cov(R, speed):
    """ "births": A = R of the row, B = 0, C = birth_speed^2 I """
    zero = np.zeros_like(R[0])
    return [R[0], R[1], R[2], zero, zero, zero, zero, zero + speed * speed, zero, zero + speed * speed]


def predict_cov(P, q_pos, q_vel):
    """ "1 predict": P = F P F^T + Q """
    axx, axz, azz, bxx, bxz, bzx, bzz, cxx, cxz, czz = P
    return [((axx + (bxx + bxx)) + cxx) + q_pos, (axz + (bxz + bzx)) + cxz, ((azz + (bzz + bzz)) + czz) + q_pos,
            bxx + cxx, bxz + cxz, bzx + cxz, bzz + czz, cxx + q_vel, cxz, czz + q_vel]


def turn_block(g, xx, xz, zx, zz):
    """ "ego": a 2 x 2 block X -> Rg X Rg^T with g = (g00, g01, g10, g11): (Rg X) first, then (Rg X) Rg^T """
    g00, g01, g10, g11 = g
    mxx, mxz = (g00 * xx) + (g01 * zx), (g00 * xz) + (g01 * zz)
    mzx, mzz = (g10 * xx) + (g11 * zx), (g10 * xz) + (g11 * zz)
    return (mxx * g00) + (mxz * g01), (mxx * g10) + (mxz * g11), (mzx * g00) + (mzz * g01), (mzx * g10) + (mzz * g11)


def turn_cov(P, g):
    """ "1b": the ground part of the ego record's rotation on the blocks A, B and C (the lower triangle of a symmetric block is not kept) """
    axx, axz, _, azz = turn_block(g, P[0], P[1], P[1], P[2])
    cxx, cxz, _, czz = turn_block(g, P[7], P[8], P[8], P[9])
    return [axx, axz, azz] + list(turn_block(g, P[3], P[4], P[5], P[6])) + [cxx, cxz, czz]


def innovation(A, R):
    """ S = A + R from the first three words of a predicted covariance and a row's noise -> (Sxx, Sxz, Szz, det) """
    sxx, sxz, szz = A[0] + R[0], A[1] + R[1], A[2] + R[2]
    return sxx, sxz, szz, (sxx * szz) - (sxz * sxz)


def update(mean, P, R, dx, dz):
    """ "5 update" of the predicted mean (x, z, vx, vz) and covariance P with a row of noise R that lies (dx, dz) from the predicted
    position -> (the new mean, the new P, det > 0); where det is not > 0 the words are not to be used: the caller takes its own fallback """
    x, z, vx, vz = mean
    axx, axz, azz, bxx, bxz, bzx, bzz, cxx, cxz, czz = P
    sxx, sxz, szz, det = innovation(P, R)
    ixx, ixz, izz = szz / det, -(sxz / det), sxx / det
    kxx, kxz, kzx, kzz = (axx * ixx) + (axz * ixz), (axx * ixz) + (axz * izz), (axz * ixx) + (azz * ixz), (axz * ixz) + (azz * izz)
    lxx, lxz, lzx, lzz = (bxx * ixx) + (bzx * ixz), (bxx * ixz) + (bzx * izz), (bxz * ixx) + (bzz * ixz), (bxz * ixz) + (bzz * izz)
    new_mean = [x + ((kxx * dx) + (kxz * dz)), z + ((kzx * dx) + (kzz * dz)), vx + ((lxx * dx) + (lxz * dz)), vz + ((lzx * dx) + (lzz * dz))]
    new = [axx - ((kxx * axx) + (kxz * axz)), axz - ((kxx * axz) + (kxz * azz)), azz - ((kzx * axz) + (kzz * azz)),
           bxx - ((kxx * bxx) + (kxz * bzx)), bxz - ((kxx * bxz) + (kxz * bzz)), bzx - ((kzx * bxx) + (kzz * bzx)),
           bzz - ((kzx * bxz) + (kzz * bzz)), cxx - ((lxx * bxx) + (lxz * bzx)), cxz - ((lxx * bxz) + (lxz * bzz)),
           czz - ((lzx * bxz) + (lzz * bzz))]
    return new_mean, new, det > 0.0
