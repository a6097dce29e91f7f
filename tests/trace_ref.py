"""An independent float64 brute force of ray traversal: BoundingVolumeHierarchy::intersect / any_intersect
(bvh.rs:160-302) answered without any tree, by testing every primitive of a SceneData.  It never calls the
product or the oracle.  Shared by tests/test_trace_reference.py (oracle) and tests/test_gpu_trace_kernels.py
(device).

Geometry (the scene's f32 arrays widened to f64, so the inputs are exact):

* triangles (triangle.rs:51-139): the watertight test is, up to a positive factor, the sign test of the three
  Plücker edge functions e_i = d . ((p_j - o) x (p_k - o)); all three of one sign is a hit, t = n.(p0 - o) / d.n.
  Expanded, e_i = d . (p_j x p_k) + (p_k - p_j) . (o x d), so all rays against all triangles are seven matrix
  products.  A hit needs 0 < t <= t_max (triangle.rs:126-127).
* spheres (sphere.rs:38-75): the ray goes through w2o, then the smallest root with t > 0 that is <= t_max.
* any hit: bvh.rs:269-280 — a hit on a triangle of the area light the shadow ray samples does not occlude.
* shape ids are the product's: triangles 0..nt-1, then spheres (SceneData.shape_order only permutes the build).
  `canon` maps each shape to the lowest id with exactly the same surface (duplicated triangles), whose tie is
  decided by leaf order, not geometry.

Robust or ambiguous.  f32 traversal can disagree with exact geometry only by rounding, so a ray whose answer
would survive any perturbation of that size is "robust" and must be answered exactly; the others are
"ambiguous" and are not asserted.  u = 2^-24 is the unit roundoff of binary32.  The margins:

* edges.  The f32 test forms p - o (one rounding, relative to |p - o|), shears p.xy += s * p.z with |s| <= 1
  (two roundings, magnitudes <= 2 |p - o|) and e = a.x b.y - a.y b.x (three roundings of products of the
  projected vertex offsets, which are <= diam when the ray passes through the triangle).  The absolute error
  of a projected coordinate is therefore <= 4u L with L = |t| |d| + diam (the distance to the hit point plus
  the triangle's extent), and of e_i / |E_i| (the distance of the ray to edge i, E_i that edge) <= 3u diam^2
  / |E_i| more.  The oblique projection of the shear stretches distances by at most sqrt(3) against the
  orthogonal ones computed here.  So the distance margin is
      delta_i = C u (L + diam^2 / |E_i|),  C = 16 >= 2 * sqrt(3) * (4 + 3) / 1.5,
  which grows with the ray's distance and, as a barycentric margin delta_i / h, shrinks with the triangle's
  size.  The distance used, e_i / (|d| |E_i|), is at most the true orthogonal one (|d x E| <= |d| |E|): every
  approximation here errs towards "ambiguous".
* t.  t = sum(b_i z_i) with z_i = p_i.z / d.z: rounding of the z_i and of the sum costs C u |t|, barycentric
  errors times the spread of the z_i (<= sqrt(3) diam / |d|) cost the rest.  A barycentric error is a distance
  error (the edge margin, with h_min the triangle's smallest altitude for the diam^2 term) over the altitude of
  the triangle as the ray sees it, h_p = |d.n| / (|d| diam) (the projected area over the longest edge; small at
  grazing incidence):  delta_t = C u (|t| + diam / |d| * (1 + (L + diam^2 / h_min) / h_p)).
* spheres.  In object space (o', d'; the f32 transform adds u |W| (|o| + 1), folded into A = |o'| + |W| (|o| + 1)),
  b^2 - 4ac cancels about u |d'|^2 A^2, which moves the distance h of the line from the centre by u A^2 / R
  near tangency:  delta_s = C u (A + R + A^2 / R);  a root moves by C u (|t| + (A + A^2 / w) / |d'|) with
  w = max(sqrt(R^2 - h^2), sqrt(R delta_s)) the half chord.
* A primitive is a "sure" hit if it passes with every margin against it and its t is farther than delta_t from
  0 and from t_max (relative u t_max more for the t_max * det product); a "maybe" hit if it passes with the
  margins in its favour and its t is not below -delta_t or above t_max + delta_t.  A closest hit is robust when
  the nearest maybe hit is a sure hit and no maybe hit of another surface lies within the two t margins; a miss
  is robust when there is no maybe hit at all.  An any-hit verdict is robust when a sure hit occludes, or when no
  maybe hit does.

The margins come from this derivation alone; they are not adjusted to any observed result."""
import numpy as np

U = 2.0 ** -24
C = 16.0
CHUNK = 1 << 22  # rays x triangles per block of the brute force's screening pass


class TraceRef:
    def __init__(self, sd):
        pts = np.asarray(sd.points, dtype=np.float64)
        idx = np.asarray(sd.indices, dtype=np.int64).reshape(-1, 3)
        self.nt = idx.shape[0]
        p0, p1, p2 = pts[idx[:, 0]], pts[idx[:, 1]], pts[idx[:, 2]]
        # edge i is opposite vertex i: e_i = d.(p_j x p_k) + (p_k - p_j).(o x d), (i, j, k) cyclic
        self.cross = [np.cross(p1, p2), np.cross(p2, p0), np.cross(p0, p1)]
        self.edge = [p2 - p1, p0 - p2, p1 - p0]
        self.elen = [np.linalg.norm(e, axis=1) for e in self.edge]
        self.n = np.cross(p1 - p0, p2 - p0)
        self.np0 = np.einsum("ij,ij->i", self.n, p0)
        self.diam = np.maximum(np.maximum(self.elen[0], self.elen[1]), self.elen[2])
        area2 = np.linalg.norm(self.n, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.hmin = np.where(self.diam > 0, area2 / self.diam, 0.0)
            self.proper = self.hmin > 0  # a zero-area triangle never hits (its f32 det is 0 or its edge signs differ)
            # the screening pass: e_i / |E_i| (the ray's distance to edge i, times |d|) as two matrix products
            self.cross_n = [np.where(self.proper[:, None], self.cross[i] / self.elen[i][:, None], 0.0) for i in range(3)]
            self.edge_n = [np.where(self.proper[:, None], self.edge[i] / self.elen[i][:, None], 0.0) for i in range(3)]
            self.q = np.where(self.proper, self.diam + self.diam * self.diam / np.minimum(np.minimum(self.elen[0], self.elen[1]), self.elen[2]), 0.0)
        self.lo = pts.min(axis=0) if len(pts) else np.zeros(3)
        self.hi = pts.max(axis=0) if len(pts) else np.zeros(3)
        self.tri_light = np.asarray(sd.tri_area_light, dtype=np.int64)
        self.spheres = [(np.asarray(s["w2o"], dtype=np.float64).reshape(4, 4), float(np.float32(s["radius"]))) for s in sd.spheres]
        self.n_shapes = self.nt + len(self.spheres)
        canon = np.arange(self.n_shapes)
        first = {}
        for i in range(self.nt):
            key = tuple(sorted((tuple(p0[i]), tuple(p1[i]), tuple(p2[i]))))
            canon[i] = first.setdefault(key, i)
        for k, (w, r) in enumerate(self.spheres):
            canon[self.nt + k] = first.setdefault((w.tobytes(), r), self.nt + k)
        self.canon = canon

    # ---------------------------------------------------------------- per-primitive tests
    def _tri_pairs(self, o, d, dn, j):
        """(t, dt, sure, maybe) of rays (o[k], d[k]) against triangles j[k] (one pair per row)."""
        m = np.cross(o, d)
        e = [np.einsum("ij,ij->i", d, self.cross[i][j]) + np.einsum("ij,ij->i", m, self.edge[i][j]) for i in range(3)]
        det = e[0] + e[1] + e[2]
        diam, hmin = self.diam[j], self.hmin[j]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (self.np0[j] - np.einsum("ij,ij->i", o, self.n[j])) / det
            s = np.sign(det)
            L = np.abs(t) * dn + diam
            sure = (det != 0) & self.proper[j]
            maybe = self.proper[j].copy()
            for i in range(3):
                el = self.elen[i][j]
                dist = s * e[i] / (dn * el)
                delta = C * U * (L + diam * diam / el)
                sure &= dist >= delta
                maybe &= (dist >= -delta) | (det == 0)  # a ray in the plane (t = nan): f32 rounding decides
            hp = np.abs(det) / (dn * diam)  # smallest altitude of the triangle as the ray sees it (projected along d)
            dt = C * U * (np.abs(t) + diam / dn * (1.0 + (L + diam * diam / hmin) / hp))
        # t = +-inf: parallel to the plane and off it; the f32 edge functions of such a ray have mixed signs
        maybe &= ~np.isinf(t)
        return t, dt, sure, maybe

    def _sphere(self, o, d, k):
        w, r = self.spheres[k]
        oo = o @ w[:3, :3].T + w[:3, 3]
        dd = d @ w[:3, :3].T
        a = np.einsum("ij,ij->i", dd, dd)
        dn = np.sqrt(a)
        h = np.linalg.norm(np.cross(oo, dd), axis=1) / dn
        mid = -np.einsum("ij,ij->i", oo, dd) / a
        half2 = r * r - h * h
        A = np.linalg.norm(oo, axis=1) + np.abs(w[:3, :]).sum(axis=1).max() * (np.abs(o).max(axis=1) + 1.0)
        ds = C * U * (A + r + A * A / r)
        half = np.sqrt(np.maximum(half2, 0.0)) / dn
        t0, t1 = mid - half, mid + half
        chord = np.maximum(np.sqrt(np.maximum(half2, 0.0)), np.sqrt(r * ds))
        dt0 = C * U * (np.abs(t0) + (A + A * A / chord) / dn)
        dt1 = C * U * (np.abs(t1) + (A + A * A / chord) / dn)
        # sphere.rs:66-75: t0 if t0 > 0, else t1; a t0 within its margin of 0 stays the candidate (near-zero rule)
        use0 = t0 >= -dt0
        t = np.where(use0, t0, t1)
        dt = np.where(use0, dt0, dt1)
        return t, dt, h <= r - ds, h <= r + ds

    def _pairs(self, o, d, t_max):
        """Every (ray, shape) pair that may hit: -> (ray, shape, t, dt, sure) arrays.  sure / maybe include the
        t range (0 < t <= t_max, margins against / in favour of the hit; u t_max more for the t_max * det product)."""
        n = o.shape[0]
        dn = np.linalg.norm(d, axis=1)
        # the screening pass keeps every pair within the largest margin a hit inside the scene's box can get
        far = np.linalg.norm(np.maximum(np.abs(o - self.lo), np.abs(o - self.hi)), axis=1)
        m = np.cross(o, d)
        out = []
        step = max(1, CHUNK // max(1, n))
        for lo in range(0, self.nt, step):
            hi = min(self.nt, lo + step)
            g = [d @ self.cross_n[i][lo:hi].T + m @ self.edge_n[i][lo:hi].T for i in range(3)]
            bound = (C * U) * dn[:, None] * (far[:, None] + self.q[lo:hi][None, :]) * 1.5
            mn = np.minimum(np.minimum(g[0], g[1]), g[2])
            mx = np.maximum(np.maximum(g[0], g[1]), g[2])
            ray, j = np.nonzero(((mn >= -bound) | (mx <= bound)) & self.proper[lo:hi][None, :])
            j = j + lo
            t, dt, sure, maybe = self._tri_pairs(o[ray], d[ray], dn[ray], j)
            out.append((ray, j, t, dt, sure, maybe))
        for k in range(len(self.spheres)):
            t, dt, sure, maybe = self._sphere(o, d, k)
            out.append((np.arange(n), np.full(n, self.nt + k), t, dt, sure, maybe))
        ray, j, t, dt, sure, maybe = (np.concatenate([b[c] for b in out]) for c in range(6))
        tm = t_max[ray]
        with np.errstate(invalid="ignore"):
            tol = dt + U * tm
            sure = sure & (t > dt) & ((tm == np.inf) | (t < tm - tol))
            maybe = maybe & (np.isnan(t) | ((t >= -dt) & (t <= tm + tol)))
        keep = maybe
        return ray[keep], j[keep], t[keep], dt[keep], sure[keep]

    # ---------------------------------------------------------------- queries
    def closest(self, o, d, t_max=None):
        """-> dict(shape (canonical id or -1), t (f64, inf on a miss), dt (its margin), robust, robust_t)
        robust_t: the nearest hit's t is well defined (sure, nothing nearer), though its surface may tie."""
        o = np.asarray(o, dtype=np.float64)
        d = np.asarray(d, dtype=np.float64)
        n = o.shape[0]
        t_max = np.full(n, np.inf) if t_max is None else np.asarray(t_max, dtype=np.float64)
        ray, j, t, dt, sure = self._pairs(o, d, t_max)
        nan_maybe = np.zeros(n, dtype=bool)
        nan_maybe[ray[np.isnan(t)]] = True
        fin = ~np.isnan(t)
        ray, j, t, dt, sure = ray[fin], j[fin], t[fin], dt[fin], sure[fin]
        order = np.lexsort((t, ray))
        first = order[np.r_[True, ray[order][1:] != ray[order][:-1]]] if len(order) else order
        best_id = np.full(n, -1, dtype=np.int64)
        best_t = np.full(n, np.inf)
        best_dt = np.zeros(n)
        best_sure = np.zeros(n, dtype=bool)
        best_id[ray[first]] = j[first]
        best_t[ray[first]] = t[first]
        best_dt[ray[first]] = dt[first]
        best_sure[ray[first]] = sure[first]
        canon_best = np.where(best_id >= 0, self.canon[np.maximum(best_id, 0)], -1)
        # competitors: maybe hits of another surface within the two t margins
        near = (self.canon[j] != canon_best[ray]) & (t - dt <= best_t[ray] + best_dt[ray])
        compete = np.zeros(n, dtype=bool)
        compete[ray[near]] = True
        hit = best_id >= 0
        robust_t = hit & best_sure & ~nan_maybe
        robust = np.where(hit, robust_t & ~compete, ~nan_maybe)
        return dict(shape=canon_best, t=best_t, dt=best_dt, robust=robust, robust_t=robust_t)

    def any(self, o, d, t_max, area_light=None):
        """-> dict(hit (bool), robust)"""
        o = np.asarray(o, dtype=np.float64)
        d = np.asarray(d, dtype=np.float64)
        n = o.shape[0]
        t_max = np.asarray(t_max, dtype=np.float64)
        al = np.full(n, -1, dtype=np.int64) if area_light is None else np.asarray(area_light, dtype=np.int64)
        ray, j, t, dt, sure = self._pairs(o, d, t_max)
        light = np.where(j < self.nt, self.tri_light[np.minimum(j, max(self.nt - 1, 0))], -1)
        occ = ~((al[ray] >= 0) & (light >= 0) & (light == al[ray]))  # bvh.rs:269-280
        sure_occ = np.zeros(n, dtype=bool)
        maybe_occ = np.zeros(n, dtype=bool)
        sure_occ[ray[occ & sure]] = True
        maybe_occ[ray[occ]] = True
        return dict(hit=sure_occ, robust=sure_occ | ~maybe_occ)

    def t_of(self, o, d, shape):
        """f64 t of ray i against shape[i] alone (nan where it cannot hit or shape < 0)."""
        o = np.asarray(o, dtype=np.float64)
        d = np.asarray(d, dtype=np.float64)
        shape = np.asarray(shape)
        out = np.full(o.shape[0], np.nan)
        tri = np.nonzero((shape >= 0) & (shape < self.nt))[0]
        t, dt, sure, maybe = self._tri_pairs(o[tri], d[tri], np.linalg.norm(d[tri], axis=1), shape[tri])
        out[tri] = np.where(maybe, t, np.nan)
        for k in range(len(self.spheres)):
            sel = np.nonzero(shape == self.nt + k)[0]
            t, dt, sure, maybe = self._sphere(o[sel], d[sel], k)
            out[sel] = np.where(maybe, t, np.nan)
        return out
