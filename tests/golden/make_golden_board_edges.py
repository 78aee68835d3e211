"""Crafted golden vectors for the createBoard profile AT its decision cuts, made by RUNNING the
reference (the shims of make_golden_board.py; nothing from the reference is copied):
``featureExtractor.featureExtractor`` on hand-built states, and ``createBoard.step`` /
``calc_reward`` for the physics group.  tests/golden/board.npz holds random rollouts, whose f64
positions never land on a cut; this file holds the states that do.  One env per case.

Groups (``group``):
  1  goal-distance bin f[0]: integer Pythagorean and axis offsets at 5 .. 30 under every sign, points
     numerically ON the circles of radius 5 .. 30 (half of them where floor(sqrt(fl(x^2)+fl(y^2))/5)
     and floor(np.hypot(x, y)/5) differ), the cap at 30, distance 0
  2  goal direction f[1..4]: the four diagonals at magnitudes 1..100, k*0.1, k/3 (agent at the origin:
     the literal magnitudes; agent elsewhere: the magnitude as the coordinates round it), the axes,
     goal == agent, vectors 1, 2, 4 and 1000 ulps off each diagonal
  3  density f[5..7] and the count f[11]: the agent coordinate at which one obstacle's gap crosses
     101 / 230 / 1000 (found in f64 by bisection on the reference's own distance), and 1, 2 ulps
     to either side, for ns in NS_ALL
  4  social force f[18]: gaps on a ladder around both roots of 1.5 N exp(-N/10) = 1, N = 0, N < 0,
     an obstacle on the agent, 32 obstacles inside the cut
  5  physics: a state one move from a cut and the move (index action or float delta): obstacle at
     exactly 20 and one ulp to either side, goal at exactly 15 and one ulp to either side, both at
     once (the collision wins), the clip at 0 and 100 from inside and from the border

``exact``: relativeGoalPos takes the cosine yi / np.linalg.norm((xi, yi)).  numpy's norm is
sqrt(dot(v, v)), whose last bit depends on whether the BLAS dot fuses its multiply-add; the plain
form is sqrt(fl(xi*xi) + fl(yi*yi)).  A case whose direction bin differs between the two forms is
stored with exact = False and both answers (``feat`` the reference's here, ``feat_alt`` the plain
form's); everywhere else feat_alt == feat.  The conditions asserted below: exact = False occurs only
among group 2's off-diagonal ulp neighbours, in at most 10 % of them.

Writes tests/golden/board_edges.npz.  Run:  python tests/golden/make_golden_board_edges.py
"""
import math
import os

import numpy as np

from make_golden_board import ACTIONS, OUT, features, load

NS_ALL = (0, 1, 4, 5, 6, 7, 8, 12, 13, 16, 17, 32)   # every board_kernel<MAXS> bound, odd counts for the pair split
MAXO = 32
FAR = (-20000, -20000)
# fixed in-field obstacle table (a case with ns obstacles and no crafted ones takes the first ns)
TABLE = [(int(x), int(y)) for x, y in np.random.RandomState(7).randint(0, 100, (MAXO, 2))]
AGENTS = [(0.0, 0.0), (37.0, 61.0), (64.0, 64.0), (12.5, 88.25)]
PI = math.pi


class Gen:
    def __init__(self):
        self.bp, self.fe, self.npx = load()
        self.board = self.bp.createBoard(static_obstacles=0, display=False)
        self.rows = []
        self.moves = []

    def _set(self, agent, goal, obst):
        b = self.board
        b.obstacle_list = [self.bp.Obstacle(10, xpos=int(x), ypos=int(y)) for x, y in obst]
        b.state = [(agent[0], agent[1]), (goal[0], goal[1]), b.calculate_distance(agent, goal)]
        b.state += [(o.x, o.y, o.rad) for o in b.obstacle_list]
        b.total_distance = b.calculate_distance(agent, goal)
        b.total_reward_accumulated = 0
        return b

    def add(self, group, agent, goal, obst, tag=0):
        agent = (float(agent[0]), float(agent[1]))
        goal = (float(goal[0]), float(goal[1]))
        assert len(obst) <= MAXO and all(-32768 <= v < 32768 for o in obst for v in o)
        b = self._set(agent, goal, obst)
        f = features(self.fe, b)
        alt = f.copy()
        alt[1:5] = plain_direction(goal[0] - agent[0], goal[1] - agent[1])
        self.rows.append(dict(group=group, agent=agent, goal=goal, obst=list(obst), feat=f, feat_alt=alt, tag=tag))
        return len(self.rows) - 1

    def add_move(self, agent, goal, obst, action=None, delta=None, tag=0):
        """Group 5: the state before the move as a case of its own, and the reference's step."""
        c = self.add(5, agent, goal, obst, tag)
        b = self._set(self.rows[c]["agent"], self.rows[c]["goal"], obst)
        total = b.total_distance
        mv = np.asarray(ACTIONS[action]) if action is not None else np.asarray([float(delta[0]), float(delta[1])])
        state, r, done, _ = b.step(mv)
        f = b.sensor_readings.numpy().reshape(-1).astype(np.float32)
        self.moves.append(dict(case=c, action=-1 if action is None else action,
                               delta=tuple(float(v) for v in (ACTIONS[action] if action is not None else delta)),
                               total=total, reward=float(r), done=bool(done),
                               agent=(float(state[0][0]), float(state[0][1])), feat=f))
        return self.moves[-1]


def plain_direction(xi, yi):
    """relativeGoalPos with the norm taken as sqrt(fl(xi*xi) + fl(yi*yi))."""
    nv = math.sqrt(xi * xi + yi * yi)
    c = yi / nv if nv > 0 else 0.0
    ang = np.arccos(np.clip(c, -1.0, 1.0))
    rel = np.zeros(4, np.float32)
    if ang < PI / 4:
        rel[0] = 1
    elif PI / 4 < ang < PI * 3 / 4:
        rel[1 if xi > 0 else 3] = 1
    else:
        rel[2] = 1
    return rel


def ulp_step(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def obst_for(ns):
    return TABLE[:ns]


def ns_cycle(i):
    return NS_ALL[i % len(NS_ALL)]


# ------------------------------------------------------------------ group 1
def group1(g):
    i = 0
    trip = [(3, 4), (6, 8), (9, 12), (12, 16), (15, 20), (7, 24), (18, 24)]
    offs = [(a, b) for a, b in trip] + [(b, a) for a, b in trip]
    offs += [(r, 0) for r in range(5, 31, 5)] + [(0, r) for r in range(5, 31, 5)]
    for ag in AGENTS[:3]:
        for a, b in offs:
            for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                if (a == 0 and sx < 0) or (b == 0 and sy < 0):
                    continue
                g.add(1, ag, (ag[0] + sx * a, ag[1] + sy * b), obst_for(ns_cycle(i)), tag=1)
                i += 1
    # points numerically on a circle: m cos t, m sin t, renormalised three times
    rng = np.random.RandomState(11)
    n_diff = n_same = 0
    for R in (5, 10, 15, 20, 25, 30):
        want = {True: 200, False: 200}
        while want[True] or want[False]:
            t = rng.uniform(0, 2 * PI)
            x, y = R * math.cos(t), R * math.sin(t)
            for _ in range(3):
                s = R / float(np.hypot(x, y))
                x, y = x * s, y * s
            ag = AGENTS[rng.randint(len(AGENTS))]
            goal = (ag[0] - x, ag[1] - y)
            dx, dy = ag[0] - goal[0], ag[1] - goal[1]
            differ = math.floor(math.sqrt(dx * dx + dy * dy) / 5) != math.floor(float(np.hypot(dx, dy)) / 5)
            if not want[differ]:
                continue
            want[differ] -= 1
            n_diff += differ
            n_same += not differ
            g.add(1, ag, goal, obst_for(ns_cycle(i)), tag=2 if differ else 3)
            i += 1
    # the cap at 30, and distance 0
    for ag in AGENTS[:2]:
        for d in (ulp_step(30.0, -1), 30.0, ulp_step(30.0, 1), 31.0, 100.0, 1e6, ulp_step(25.0, -1), ulp_step(5.0, -1)):
            for vx, vy in ((d, 0.0), (0.0, -d), (-d, 0.0), (0.0, d)):
                g.add(1, ag, (ag[0] + vx, ag[1] + vy), obst_for(ns_cycle(i)), tag=4)
                i += 1
    for ag in AGENTS:
        for ns in NS_ALL:
            g.add(1, ag, ag, obst_for(ns), tag=5)
    return n_diff, n_same


# ------------------------------------------------------------------ group 2
def magnitudes():
    m = [float(k) for k in range(1, 101)] + [k * 0.1 for k in range(1, 151)] + [k / 3 for k in range(1, 151)]
    return sorted(set(m))


DIAGS = ((1, 1), (-1, 1), (1, -1), (-1, -1))


def group2(g):
    i = 0
    mags = magnitudes()
    for m in mags:               # the literal magnitudes: agent at the origin
        for sx, sy in DIAGS:
            g.add(2, AGENTS[0], (sx * m, sy * m), obst_for(ns_cycle(i)), tag=1)
            i += 1
    for j, m in enumerate(mags):   # elsewhere: the magnitude both coordinates can carry exactly
        ag = AGENTS[1 + j % 3]
        q = m
        for _ in range(4):
            q = (ag[0] + q) - ag[0]
            q = (ag[1] + q) - ag[1]
        for sx, sy in DIAGS:
            goal = (ag[0] + sx * q, ag[1] + sy * q)
            if not (goal[0] - ag[0] == sx * q and goal[1] - ag[1] == sy * q):
                continue       # (the smaller coordinate cannot carry it: skip, the origin cases cover it)
            g.add(2, ag, goal, obst_for(ns_cycle(i)), tag=1)
            i += 1
    for ag in AGENTS:           # the axes, and goal == agent
        for m in (1.0, 0.1, 1 / 3, 50.0, 99.9):
            for vx, vy in ((m, 0.0), (0.0, m), (-m, 0.0), (0.0, -m)):
                g.add(2, ag, (ag[0] + vx, ag[1] + vy), obst_for(ns_cycle(i)), tag=2)
                i += 1
        g.add(2, ag, ag, obst_for(ns_cycle(i)), tag=3)
        i += 1
    first = len(g.rows)
    rng = np.random.RandomState(13)
    for m in [mags[k] for k in sorted(rng.choice(len(mags), 56, replace=False))]:
        for sx, sy in DIAGS:
            for k in (1, 2, 4, 1000):
                for side in (1, -1):
                    g.add(2, AGENTS[0], (sx * m, sy * ulp_step(m, side * k)), obst_for(ns_cycle(i)), tag=4)
                    i += 1
    return first, len(g.rows)


# ------------------------------------------------------------------ group 3
def ref_gap(fe, bp, agent, o):
    return float(fe.calcDistance(bp.Obstacle(10, xpos=o[0], ypos=o[1]), agent, 10))


def plain_gap(agent, o):
    dx, dy = o[0] - agent[0], o[1] - agent[1]
    return math.sqrt(dx * dx + dy * dy) - 10 - 20


def flip_point(g, o, ay, cut, lo, hi):
    """Adjacent doubles (a, b), lo <= a < b <= hi, with gap(a) < cut and not gap(b) < cut (the gap
    grows with the agent's x moving away from the obstacle at o)."""
    inside = lambda x: ref_gap(g.fe, g.bp, (x, ay), o) < cut   # noqa: E731
    assert inside(lo) and not inside(hi), (o, ay, cut)
    while math.nextafter(lo, hi) != hi:
        mid = lo + (hi - lo) / 2
        if inside(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def group3(g):
    # (cut, obstacle, agent y, bracket of agent x: inside first); dy is an integer, so the square the
    # norm's dot product may fuse is exact and both forms of the norm agree
    setups = [(101, (-60, 50), 50.0, 70.0, 72.0), (101, (-20, -30), 50.0, 80.0, 90.0),
              (230, (-200, 40), 40.0, 59.0, 61.0), (230, (-60, 251), 10.0, 10.0, 50.0),
              (1000, (-1000, 77), 77.0, 29.0, 31.0), (1000, (-850, -500), 20.5, 1.0, 60.0)]
    n = 0
    for cut, o, ay, lo, hi in setups:
        a, b = flip_point(g, o, ay, cut, lo, hi)
        xs = [ulp_step(a, -2), ulp_step(a, -1), a, b, ulp_step(b, 1), ulp_step(b, 2)]
        for x in xs:
            assert (ref_gap(g.fe, g.bp, (x, ay), o) < cut) == (plain_gap((x, ay), o) < cut), (cut, o, x)
        for ns in NS_ALL:
            for x in xs:
                goal = (90.0, 5.0)
                if ns == 0:
                    g.add(3, (x, ay), goal, [], tag=cut)
                    continue
                g.add(3, (x, ay), goal, obst_for(ns - 1) + [o], tag=cut)    # the last slot
                g.add(3, (x, ay), goal, [o] * ns, tag=cut)                  # every slot: the count flips 0 <-> ns
                n += 2
    return n


# ------------------------------------------------------------------ group 4
def force_root(lo, hi):
    f = lambda N: 1.5 * N * math.exp(-N / 10) - 1   # noqa: E731
    s = f(lo) < 0
    for _ in range(200):
        mid = (lo + hi) / 2
        if (f(mid) < 0) == s:
            lo = mid
        else:
            hi = mid
    return lo


def group4(g):
    i = 0
    roots = (force_root(0.1, 5.0), force_root(20.0, 60.0))
    assert abs(roots[0] - 0.71616) < 1e-4 and abs(roots[1] - 41.2515) < 1e-3, roots
    near = 0
    for root in roots:
        for e in (1e-3, 1e-6, 1e-9, 1e-12):
            for s in (1, -1):
                N = root * (1 + s * e)
                for ay, o in ((50.0, (10, 50)), (33.0, (2, 33))):
                    ax = o[0] + (N + 30.0)
                    for ns in ((1, 6, 13, 32) if e == 1e-12 else (NS_ALL[1 + i % 11],)):
                        got = ref_gap(g.fe, g.bp, (ax, ay), o)
                        f = 1.5 * got * math.exp(-got / 10)
                        if abs(f - 1.0) <= 4 * 2.0 ** -52:
                            near += 1
                            continue
                        g.add(4, (ax, ay), (5.0, 95.0), [FAR] * (ns - 1) + [o], tag=1)
                        g.add(4, (ax, ay), (5.0, 95.0), [o] * ns, tag=1)
                        i += 1
    assert near == 0, near
    for ag in AGENTS[1:]:
        ix, iy = int(ag[0]), int(ag[1])
        a0 = (float(ix), float(iy))
        for ns in (1, 5, 8, 12, 17):
            g.add(4, a0, (5.0, 95.0), [(ix + 18, iy + 24)] * ns, tag=2)                     # N = 0
            g.add(4, a0, (5.0, 95.0), obst_for(ns - 1) + [(ix - 18, iy - 24)], tag=2)
            g.add(4, a0, (5.0, 95.0), [(ix + 3, iy + 4)] * ns, tag=3)                       # N < 0
            g.add(4, a0, (5.0, 95.0), obst_for(ns - 1) + [(ix, iy)], tag=4)                 # on the agent
            g.add(4, a0, (5.0, 95.0), [(ix, iy)] * ns, tag=4)
    rng = np.random.RandomState(17)
    for ag in ((50.3, 49.6), (41.7, 58.1), (50.0, 50.0), (55.55, 44.45)):                  # all inside the cut
        ring = []
        while len(ring) < MAXO:
            x, y = rng.randint(-20, 120, 2)
            if 31.0 < math.hypot(x - ag[0], y - ag[1]) < 65.0:
                ring.append((int(x), int(y)))
        for ns in (32, 17, 16, 13, 7):
            g.add(4, ag, (5.0, 95.0), ring[:ns], tag=5)


# ------------------------------------------------------------------ group 5
def delta_to(start, target):
    d = target - start
    assert start + d == target, (start, target)
    return d


def group5(g):
    far_goal = (95.0, 3.0)
    for ns in NS_ALL[1:]:
        for slot in sorted({0, ns - 1, ns // 2}):
            def obs(o):
                lst = [FAR] * ns
                lst[slot] = o
                return lst
            ox, oy = 30, 40
            # obstacle distance exactly 20 after the move: axis (index action), 12-16-20 (index action)
            g.add_move((ox + 21.0, oy), far_goal, obs((ox, oy)), action=3, tag=1)
            g.add_move((ox + 12.0, oy + 17.0), far_goal, obs((ox, oy)), action=0, tag=1)
            g.add_move((ox + 22.0, oy), far_goal, obs((ox, oy)), action=3, tag=1)          # 21: no hit
            for k in (-1, 0, 1):                                                             # float deltas
                t = ulp_step(ox + 20.0, k)
                g.add_move((ox + 21.0, oy), far_goal, obs((ox, oy)), delta=(delta_to(ox + 21.0, t), 0.0), tag=1)
                t = ulp_step(oy - 20.0, k)
                g.add_move((ox, oy - 20.75), far_goal, obs((ox, oy)), delta=(0.0, delta_to(oy - 20.75, t)), tag=1)
            # collision and goal at once: 20 from the obstacle, 9 from the goal
            g.add_move((ox + 21.0, oy), (ox + 20.0, oy + 9.0), obs((ox, oy)), action=3, tag=3)
            g.add_move((ox + 20.5, oy), (ox + 14.0, oy + 12.0), obs((ox, oy)), delta=(-0.5, 0.0), tag=3)
    for ns in NS_ALL:            # goal distance exactly 15 after the move, and one ulp to either side
        ob = [FAR] * ns
        for ag in ((50.0, 50.0), (20.0, 70.5)):
            g.add_move((ag[0] + 1.0, ag[1]), (ag[0] + 15.0, ag[1]), ob, action=3, tag=2)    # 15: not < 15
            g.add_move((ag[0], ag[1] + 1.0), (ag[0] + 9.0, ag[1] + 12.0), ob, action=0, tag=2)
            g.add_move((ag[0] - 1.0, ag[1]), (ag[0] + 14.0, ag[1]), ob, action=1, tag=2)    # 14
            for k in (-1, 0, 1):
                t = ulp_step(ag[0] + 15.0, k)
                g.add_move((ag[0] + 16.0, ag[1]), (ag[0], ag[1]), ob, delta=(delta_to(ag[0] + 16.0, t), 0.0), tag=2)
                t = ulp_step(ag[1] - 15.0, k)
                g.add_move((ag[0], ag[1] - 15.5), (ag[0], ag[1]), ob, delta=(0.0, delta_to(ag[1] - 15.5, t)), tag=2)
    for ns in (0, 5, 13, 32):    # the clip at 0 and 100: from inside and from exactly on the border
        ob = [FAR] * ns
        goal = (50.0, 50.0)
        for a in range(4):
            dx, dy = ACTIONS[a]
            for edge in (0.0, 100.0):
                for inset in (0.0, 0.5, 1.0):
                    c = edge + inset if edge == 0.0 else edge - inset
                    g.add_move((c, 80.0) if dx else (80.0, c), goal, ob, action=a, tag=4)
        for d in ((-0.7, 0.0), (0.7, 0.0), (0.0, -0.7), (0.0, 0.7), (-250.0, 300.0), (1e-300, -1e-300)):
            for ag in ((0.0, 100.0), (100.0, 0.0), (0.3, 99.7), (99.7, 0.3), (0.7, 99.3)):
                g.add_move(ag, goal, ob, delta=d, tag=4)


def main():
    g = Gen()
    n_diff, n_same = group1(g)
    nb0, nb1 = group2(g)
    group3(g)
    group4(g)
    group5(g)
    rows, moves = g.rows, g.moves
    C = len(rows)
    exact = np.array([np.array_equal(r["feat"], r["feat_alt"]) for r in rows])
    group = np.array([r["group"] for r in rows], np.int8)
    neigh = np.zeros(C, bool)
    neigh[nb0:nb1] = True
    assert not (~exact & ~neigh).any(), "exact = False outside group 2's off-diagonal neighbours"
    share = float((~exact & neigh).sum()) / int(neigh.sum())
    assert share <= 0.10, share
    obst = np.full((C, MAXO, 2), 0, np.int16)
    ns = np.zeros(C, np.int8)
    for c, r in enumerate(rows):
        ns[c] = len(r["obst"])
        if r["obst"]:
            obst[c, :len(r["obst"])] = r["obst"]
    d = dict(agent=np.array([r["agent"] for r in rows]), goal=np.array([r["goal"] for r in rows]), obst=obst, ns=ns,
             feat=np.stack([r["feat"] for r in rows]), feat_alt=np.stack([r["feat_alt"] for r in rows]),
             group=group, tag=np.array([r["tag"] for r in rows], np.int16), exact=exact,
             mv_case=np.array([m["case"] for m in moves], np.int32),
             mv_action=np.array([m["action"] for m in moves], np.int8),
             mv_delta=np.array([m["delta"] for m in moves]), mv_total=np.array([m["total"] for m in moves]),
             mv_reward=np.array([m["reward"] for m in moves]), mv_done=np.array([m["done"] for m in moves], np.uint8),
             mv_agent=np.array([m["agent"] for m in moves]), mv_feat=np.stack([m["feat"] for m in moves]))
    path = os.path.join(OUT, "board_edges.npz")
    np.savez_compressed(path, **d)
    print("cases", C, "by group", {k: int((group == k).sum()) for k in range(1, 6)}, "moves", len(moves))
    print("group 1 on-circle points: sqrt form and hypot floor differently", n_diff, "agree", n_same)
    print("group 2 off-diagonal neighbours", int(neigh.sum()), "exact = False", int((~exact).sum()),
          f"({100 * share:.1f} %), elsewhere", int((~exact & ~neigh).sum()))
    up = (group == 2) & (d["tag"] == 1) & (d["goal"][:, 1] > d["agent"][:, 1])
    print("group 2 up-diagonal cases", int(up.sum()), "ahead", int(d["feat"][up, 1].sum()), "side",
          int(d["feat"][up][:, [2, 4]].sum()), "behind", int(d["feat"][up, 3].sum()))
    mv_r = d["mv_reward"]
    print("moves: hits", int((mv_r == -1).sum()), "goals", int((mv_r == 1).sum()), "neither", int((d["mv_done"] == 0).sum()))
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
