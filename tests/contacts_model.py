"""numpy model of the contact row of include/ftgp.h (FTGP_CONTACT_FLOATS): the header's text, operation by operation in binary64, and
nothing of the library's.  Every numpy operation below is one IEEE operation per element (numpy fuses nothing), so a float32 rounding
of the result is what the library must write, to the bit.

    contact_rows(track, vehicle, pose, finished, cpe, bubble)      float32 [n, 4]: wall_pen, car_pen, wall_count, car_count
    contact_rows64(...)                                            the same before the rounding, and which mate slots each car overlaps

pose: rows of ftgp_get_pose (x, y at 0, 1; qw, qz at 3, 6); finished: per car, non-zero = has finished; the cars of an env are
consecutive rows, `cpe` of them; the track is the one of every env handed in (a multi-track handle: one call per block).
"""
import math

import numpy as np

CONTACT_FLOATS = 4
WALL_PEN, CAR_PEN, WALL_COUNT, CAR_COUNT = range(4)


def heading(pose):
    """(ch, sh) as K1 writes them."""
    qw, qz = pose[:, 3], pose[:, 6]
    return 1.0 - 2.0 * (qz * qz), 2.0 * (qw * qz)


def wall_circles(v, bubble):
    """(body x, body y, radius, softener) of a car's wall circles: three on the axis, with bubble_wrap four more at the wheels."""
    c = [(v.contact_x[k], 0.0, v.contact_radius, False) for k in range(3)]
    if bubble:
        c += [(v.wheel_x[k], v.wheel_y[k], v.softener_radius, True) for k in range(4)]
    return c


def circle_against_walls(t, wall, px, py, r):
    """(touches [m] bool, penetration [m]) of circles of radius r centred at (px, py) [m] on the image of track t."""
    W, H, sx, sy, ox, oy = t.width, t.height, float(t.px_size_x), float(t.px_size_y), float(t.origin_x), float(t.origin_y)
    inv_x, inv_y = 1.0 / sx, 1.0 / sy
    nx, ny = int(math.ceil(r * inv_x)), int(math.ceil(r * inv_y))
    with np.errstate(invalid="ignore"):
        u, w = (px - ox) * inv_x, (oy - py) * inv_y
        fu, fw = np.floor(u), np.floor(w)
        on_image = np.isfinite(fu) & np.isfinite(fw) & (fu >= 0) & (fu < W) & (fw >= 0) & (fw < H)
    ix, iy = np.where(on_image, fu, 0).astype(np.int64), np.where(on_image, fw, 0).astype(np.int64)
    cx = ix[:, None, None] + np.arange(-nx, nx + 1)[None, None, :]
    cy = iy[:, None, None] + np.arange(-ny, ny + 1)[None, :, None]
    cx, cy = np.broadcast_arrays(cx, cy)
    pixel = on_image[:, None, None] & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    pixel = pixel & wall[np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
    x0 = ox + cx.astype(np.float64) * sx
    x1 = x0 + sx
    y1 = oy - cy.astype(np.float64) * sy
    y0 = y1 - sy
    PX, PY = px[:, None, None], py[:, None, None]
    with np.errstate(invalid="ignore"):
        qx = np.where(PX < x0, x0, np.where(PX > x1, x1, PX))
        qy = np.where(PY < y0, y0, np.where(PY > y1, y1, PY))
        ex, ey = PX - qx, PY - qy
        d2 = ex * ex + ey * ey
        touch = pixel & (d2 < r * r)
        pen = np.where(touch, r - np.sqrt(np.where(touch, d2, 0.0)), -np.inf)
    found = touch.any(axis=(1, 2))
    return found, np.where(found, pen.max(axis=(1, 2)), 0.0)


def contact_rows64(track, vehicle, pose, finished, cpe, bubble):
    """(rows float64 [n, 4], mates bool [n, cpe]: car a overlaps the car in slot k of its env)."""
    pose = np.asarray(pose, dtype=np.float64)
    n, v = len(pose), vehicle
    assert n % cpe == 0
    racing = np.asarray(finished).reshape(n) == 0
    wall = track.wall_mask()
    x, y = pose[:, 0], pose[:, 1]
    ch, sh = heading(pose)
    rows = np.zeros((n, CONTACT_FLOATS))
    # walls
    wall_pen, wall_count = np.zeros(n), np.zeros(n, dtype=np.int64)
    for bx, by, r, softener in wall_circles(v, bubble):
        if softener:
            px, py = x + (ch * bx - sh * by), y + (sh * bx + ch * by)
        else:
            px, py = x + ch * bx, y + sh * bx
        found, pen = circle_against_walls(track, wall, px, py, float(r))
        found = found & racing
        wall_pen = np.where(found & (pen > wall_pen), pen, wall_pen)
        wall_count += found
    # env-mates
    r2 = 2.0 * v.contact_radius
    E = n // cpe
    X, Y, CH, SH, R = (a.reshape(E, cpe) for a in (x, y, ch, sh, racing))
    car_pen, mates = np.zeros((E, cpe)), np.zeros((E, cpe, cpe), dtype=bool)
    for a in range(cpe):
        for b in range(cpe):
            if a == b:
                continue
            both = R[:, a] & R[:, b]
            for i in range(3):
                for j in range(3):
                    px, py = X[:, a] + CH[:, a] * v.contact_x[i], Y[:, a] + SH[:, a] * v.contact_x[i]
                    qx, qy = X[:, b] + CH[:, b] * v.contact_x[j], Y[:, b] + SH[:, b] * v.contact_x[j]
                    ex, ey = px - qx, py - qy
                    d2 = ex * ex + ey * ey
                    with np.errstate(invalid="ignore"):
                        counts = both & (d2 > 0.0) & (d2 < r2 * r2)
                        overlap = r2 - np.sqrt(np.where(counts, d2, 0.0))
                    car_pen[:, a] = np.where(counts & (overlap > car_pen[:, a]), overlap, car_pen[:, a])
                    mates[:, a, b] |= counts
    rows[:, WALL_PEN], rows[:, CAR_PEN] = wall_pen, car_pen.reshape(n)
    rows[:, WALL_COUNT], rows[:, CAR_COUNT] = wall_count, mates.sum(axis=2).reshape(n)
    return rows, mates.reshape(n, cpe)


def contact_rows(track, vehicle, pose, finished, cpe, bubble):
    return contact_rows64(track, vehicle, pose, finished, cpe, bubble)[0].astype(np.float32)


def contact_rows_blocks(tracks, envs_per_track, vehicle, pose, finished, cpe, bubble):
    """A multi-track handle: block t = envs_per_track[t] consecutive envs against tracks[t]'s frame."""
    out, a = [], 0
    for t, envs in zip(tracks, envs_per_track):
        b = a + envs * cpe
        out.append(contact_rows(t, vehicle, pose[a:b], np.asarray(finished)[a:b], cpe, bubble))
        a = b
    return np.concatenate(out)
