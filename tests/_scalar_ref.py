"""The passive scalar of include/lbm.h ("Scalar transport") restated in numpy float64: the reference the GPU tests compare bits
against, the flows with known answers that hold it to the physics, and their figures.

step() is the header's statements, one ufunc per written operator in the header's order (numpy never contracts two ufunc calls
into an FMA).  The velocity a scalar step reads is _drive_ref.fields (the output stage, with the body force the physical velocity)
on the state the flow's step streams: the stored state after accelerate() where the flow is periodic, the stored state itself with
open boundaries on.  The flow's own step is the existing reference (_drive_ref.step and what it routes to), imported and not
edited.  advance() is one scalar step followed by one flow step, the order of the library's stream."""
from types import SimpleNamespace

import numpy as np

import _drive_ref

CX = [0, 1, 0, -1, 0]
CY = [0, 0, 1, 0, -1]
OPP = [0, 3, 4, 1, 2]
THIRD, SIXTH = np.float64(1.0) / np.float64(3.0), np.float64(1.0) / np.float64(6.0)
THREE = np.float64(3.0)
WEIGHTS = [THIRD, SIXTH, SIXTH, SIXTH, SIXTH]


def omega_s(diffusivity):
    """the header's host statement"""
    return np.float64(1.0) / (np.float64(3.0) * np.float64(diffusivity) + np.float64(0.5))


def init(c0):
    """g[k] = w_k * c0 on every cell"""
    c0 = np.asarray(c0, dtype=np.float64)
    return np.stack([w * c0 for w in WEIGHTS])


def field(g, ob):
    """the reported field: the sum of a fluid cell's five stored values, 0.0 on a blocked cell"""
    c = (((g[0] + g[1]) + g[2]) + g[3]) + g[4]
    return np.where(ob != 0, 0.0, c)


def step(g, ob, u_x, u_y, om_s, c_wall=None, c_in=None):
    """One scalar step of the stored populations g[5, ny, nx] under the velocities u_x, u_y of the fluid cells.  c_wall: None (all
    insulating) or [ny, nx] with NaN = insulating; c_in: None (the flow is periodic) or [ny], open boundaries on."""
    assert g.dtype == np.float64 and g.shape[0] == 5
    ny, nx = ob.shape
    blocked = ob != 0
    wall = np.full((ny, nx), np.nan) if c_wall is None else np.asarray(c_wall, dtype=np.float64)
    om_s = np.float64(om_s)
    with np.errstate(all="ignore"):                       # blocked cells go through the arithmetic and are replaced below
        h = [g[0]]
        for k in range(1, 5):
            shift = (CY[k], CX[k])                        # the value at q = x - c_k
            q_blocked = np.roll(blocked, shift, axis=(0, 1))
            q_wall = np.roll(wall, shift, axis=(0, 1))
            back = g[OPP[k]]
            held = THIRD * q_wall - back
            h.append(np.where(q_blocked, np.where(np.isnan(q_wall), back, held), np.roll(g[k], shift, axis=(0, 1))))
        if c_in is not None:
            h[1] = h[1].copy()
            h[3] = h[3].copy()
            h[1][:, 0] = np.asarray(c_in, dtype=np.float64) - (((h[0][:, 0] + h[2][:, 0]) + h[3][:, 0]) + h[4][:, 0])
            h[3][:, nx - 1] = g[3][:, nx - 1]
        c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4]
        a_x = THREE * (c * u_x)
        a_y = THREE * (c * u_y)
        e = [THIRD * c, SIXTH * (c + a_x), SIXTH * (c + a_y), SIXTH * (c - a_x), SIXTH * (c - a_y)]
        out = [h[k] + om_s * (e[k] - h[k]) for k in range(5)]
    return np.stack([np.where(blocked, g[k], out[k]) for k in range(5)])


def accelerate(f, ob, density, accel):
    """accelerate_flow on row ny - 2 (dp_accelerate_cell): fluid, and none of the three west-side values would go negative"""
    ny = ob.shape[0]
    aw1 = np.float64(density) * np.float64(accel) / np.float64(9.0)
    aw2 = np.float64(density) * np.float64(accel) / np.float64(36.0)
    f = np.array(f, dtype=np.float64, copy=True)
    r = f[:, ny - 2]
    ok = (ob[ny - 2] == 0) & ((r[3] - aw1) > 0.0) & ((r[6] - aw2) > 0.0) & ((r[7] - aw2) > 0.0)
    for k, a in ((1, aw1), (5, aw2), (8, aw2)):
        r[k] = np.where(ok, r[k] + a, r[k])
    for k, a in ((3, aw1), (6, aw2), (7, aw2)):
        r[k] = np.where(ok, r[k] - a, r[k])
    return f


def velocity(f, ob, drive=None):
    """(u_x, u_y) of the output stage on the state f: what a scalar step reads on the fluid cells"""
    u_x, u_y = _drive_ref.fields(f, ob, 1.0, drive)[:2]
    return u_x, u_y


def flow(ob, density=0.1, accel=0.0, omega=1.0, magic=None, opened=None, drive=None):
    """what advance() needs of a flow: opened = None or (u_in[ny], rho_out)"""
    return SimpleNamespace(ob=ob, density=density, accel=accel, omega=omega, magic=magic, opened=opened, drive=drive)


def streamed(f, fl):
    """the state the flow's next step streams"""
    return f if fl.opened is not None else accelerate(f, fl.ob, fl.density, fl.accel)


def flow_step(fa, fl):
    u_in, rho_out = fl.opened if fl.opened is not None else (None, None)
    return _drive_ref.step(fa, fl.ob, fl.omega, fl.magic, u_in, rho_out, drive=fl.drive)[0]


def advance(f, g, fl, om_s, c_wall=None, c_in=None):
    """scalar step n, then flow step n: (f, g) after it"""
    fa = streamed(f, fl)
    u_x, u_y = velocity(fa, fl.ob, fl.drive)
    g = step(g, fl.ob, u_x, u_y, om_s, c_wall, c_in if fl.opened is not None else None)
    return flow_step(fa, fl), g


def rest(ob, density=0.1):
    from _open_ref import rest_state
    return rest_state(density, *ob.shape).copy()


# ---- the flows with known answers ------------------------------------------------------------------------------------------
# Each has a setup (mask, flow, first states, scalar arguments) shared by tests/golden/make_scalar.py, the CPU module and the GPU
# module, and a function that turns fields into the figures the gates are about.

DENSITY = 0.1
START = 200          # steps of every flow that the CPU module recomputes

CONSERVATION = dict(nx=32, ny=32, accel=0.005, omega=1.0, D=0.05, steps=200, every=50, gate=1e-12)
DIFFUSION = dict(nx=32, ny=32, steps=200, every=20, Ds=(0.02, 0.05, 0.2), gate=0.03)
WALLS = dict(nx=4, ny=18, Ds=(0.02, 0.1, 1.0 / 6.0, 0.3), gate=1e-10)
OPEN = dict(nx=64, ny=4, u_in=0.05, rho_out=0.1, Ds=(0.01, 0.05), steps=6000, gate=1e-10)
TAYLOR = dict(nx=1024, ny=18, omega=1.0, magic=3.0 / 16.0, u_mean=0.05, spin_up=6000, D=0.08, sigma=6.0, t0=9600, t1=16000,
              gate=0.05, speed_gate=0.01, parabola_gate=1e-9)


def wave(nx, ny):
    """c0 = 1 + 0.5 sin(kx) cos(ky), k = 2 pi / 32 on the 32 x 32 grids"""
    k = 2.0 * np.pi / 32.0
    y, x = np.mgrid[0:ny, 0:nx]
    return 1.0 + 0.5 * np.sin(k * x) * np.cos(k * y)


def conservation_mask():
    """32 x 32, periodic: a wall segment, a block and isolated cells, all insulating"""
    ob = np.zeros((32, 32), dtype=np.int32)
    ob[5, 3:20] = 1
    ob[14:19, 9:14] = 1
    for y, x in ((2, 28), (24, 6), (27, 27), (30, 15), (11, 25)):
        ob[y, x] = 1
    return ob


def conservation_setup():
    c = CONSERVATION
    ob = conservation_mask()
    return SimpleNamespace(ob=ob, fl=flow(ob, DENSITY, c["accel"], c["omega"]), c0=wave(c["nx"], c["ny"]), D=c["D"])


def total(c, ob):
    """the sum of the field over the fluid cells"""
    return float(np.sum(c[ob == 0]))


def walls_steps(D):
    return int(round(8 * 16 ** 2 / D))


def walls_setup():
    nx, ny = WALLS["nx"], WALLS["ny"]
    ob = _drive_ref.channel_mask(nx, ny)
    wall = np.full((ny, nx), np.nan)
    wall[0], wall[ny - 1] = 1.0, 0.0
    return SimpleNamespace(ob=ob, fl=flow(ob, DENSITY, 0.0, 1.0), c0=np.zeros((ny, nx)), wall=wall)


def walls_figure(c):
    """max |C - (1 - (y - 1/2) / 16)| over the fluid rows 1 .. 16"""
    ny = c.shape[0]
    y = np.arange(1, ny - 1, dtype=np.float64)
    return float(np.max(np.abs(c[1:ny - 1] - (1.0 - (y - 0.5) / 16.0)[:, None])))


def diffusion_amplitude(c):
    """the amplitude of sin(kx) cos(ky) in the field of the 32 x 32 grid"""
    ny, nx = c.shape
    mode = (wave(nx, ny) - 1.0) / 0.5
    return float(np.sum((c - 1.0) * mode) / np.sum(mode * mode))


def diffusion_rate(times, amplitudes):
    """the decay rate fitted to ln A(t) by least squares"""
    return float(-np.polyfit(np.asarray(times, dtype=np.float64), np.log(np.asarray(amplitudes, dtype=np.float64)), 1)[0])


def diffusion_theory(D):
    k = 2.0 * np.pi / 32.0
    return 2.0 * D * k * k


def uniform_equilibrium(nx, ny, rho, u):
    """the D2Q9 equilibrium of density rho and velocity (u, 0) on every cell"""
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
    cx = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.float64)
    eq = w * rho * (1.0 + 3.0 * cx * u + 4.5 * (cx * u) ** 2 - 1.5 * u * u)
    return np.ascontiguousarray(np.broadcast_to(eq.reshape(9, 1, 1), (9, ny, nx)))


def open_setup():
    o = OPEN
    ob = np.zeros((o["ny"], o["nx"]), dtype=np.int32)
    u_in = np.full(o["ny"], o["u_in"])
    return SimpleNamespace(ob=ob, fl=flow(ob, DENSITY, 0.0, 1.0, opened=(u_in, o["rho_out"])),
                           f0=uniform_equilibrium(o["nx"], o["ny"], o["rho_out"], o["u_in"]), c0=np.zeros((o["ny"], o["nx"])),
                           inlet=np.ones(o["ny"]))


def taylor_force():
    """the force density whose parabola between walls half-way has the mean TAYLOR['u_mean']: F H^2 / (12 rho nu)"""
    t = TAYLOR
    h = float(t["ny"] - 2)
    nu = (1.0 / t["omega"] - 0.5) / 3.0
    return 12.0 * DENSITY * nu * t["u_mean"] / (h * h)


def taylor_setup():
    t = TAYLOR
    ob = _drive_ref.channel_mask(t["nx"], t["ny"])
    x = np.arange(t["nx"], dtype=np.float64)
    c0 = np.broadcast_to(np.exp(-0.5 * ((x - 128.0) / t["sigma"]) ** 2), (t["ny"], t["nx"])).copy()
    return SimpleNamespace(ob=ob, fl=flow(ob, DENSITY, 0.0, t["omega"], t["magic"], drive=(taylor_force(), 0.0)), c0=c0, x0=128.0)


def taylor_parabola_deviation(u_x, pressure):
    """max |u_x - parabola| / max parabola over the fluid rows, the parabola at the mean density (test_drive_gpu's figure)"""
    t = TAYLOR
    return _drive_ref.poiseuille_figures(u_x, np.zeros_like(u_x), pressure, t["omega"], taylor_force())[0]


def taylor_moments(c, steps):
    """(centre, variance) of the cross-section mean of the field after `steps` scalar steps, unwrapped about the moving centre"""
    t = TAYLOR
    ny, nx = c.shape
    m = c[1:ny - 1].mean(axis=0)
    guess = 128.0 + t["u_mean"] * steps
    dx = (np.arange(nx, dtype=np.float64) - guess + nx / 2.0) % nx - nx / 2.0
    mass = float(np.sum(m))
    mu = float(np.sum(m * dx)) / mass
    return guess + mu, float(np.sum(m * (dx - mu) ** 2)) / mass


def taylor_figures(c_t0, c_t1):
    """(D_eff over theory, centre speed over u_mean) from the fields at steps t0 and t1"""
    t = TAYLOR
    x0, v0 = taylor_moments(c_t0, t["t0"])
    x1, v1 = taylor_moments(c_t1, t["t1"])
    dt = float(t["t1"] - t["t0"])
    pe = t["u_mean"] * (t["ny"] - 2) / t["D"]
    theory = t["D"] * (1.0 + pe * pe / 210.0)
    return (v1 - v0) / (2.0 * dt) / theory, (x1 - x0) / dt / t["u_mean"]


# ---- one description per run, for the fixture's generator and the two test modules ---------------------------------------------

def case(kind, D=None):
    """The run `kind` at diffusivity D: ob, fl (flow()), f0 (the flow state the run starts from; taylor: the state from which its
    spin-up starts), spin_up (flow steps before the scalar is set), c0, wall, inlet, steps (scalar steps), samples (the steps
    after which the field is looked at)."""
    if kind == "conservation":
        s = conservation_setup()
        c = CONSERVATION
        return SimpleNamespace(ob=s.ob, fl=s.fl, f0=rest(s.ob), spin_up=0, c0=s.c0, D=c["D"], wall=None, inlet=None, steps=c["steps"],
                               samples=list(range(c["every"], c["steps"] + 1, c["every"])))
    if kind == "diffusion":
        d = DIFFUSION
        ob = np.zeros((d["ny"], d["nx"]), dtype=np.int32)
        return SimpleNamespace(ob=ob, fl=flow(ob, DENSITY, 0.0, 1.0), f0=rest(ob), spin_up=0, c0=wave(d["nx"], d["ny"]), D=D, wall=None,
                               inlet=None, steps=d["steps"], samples=list(range(d["every"], d["steps"] + 1, d["every"])))
    if kind == "walls":
        s = walls_setup()
        n = walls_steps(D)
        return SimpleNamespace(ob=s.ob, fl=s.fl, f0=rest(s.ob), spin_up=0, c0=s.c0, D=D, wall=s.wall, inlet=None, steps=n, samples=[n])
    if kind == "open":
        s = open_setup()
        return SimpleNamespace(ob=s.ob, fl=s.fl, f0=s.f0.copy(), spin_up=0, c0=s.c0, D=D, wall=None, inlet=s.inlet, steps=OPEN["steps"],
                               samples=[OPEN["steps"]])
    assert kind == "taylor"
    s = taylor_setup()
    t = TAYLOR
    return SimpleNamespace(ob=s.ob, fl=s.fl, f0=rest(s.ob), spin_up=t["spin_up"], c0=s.c0, D=t["D"], wall=None, inlet=None, steps=t["t1"],
                           samples=[t["t0"], t["t1"]])


def run(cs, steps=None, spin_up=None):
    """The run of case(): (flow state at the end, {step: field} at the samples reached, field after the last step)"""
    f = cs.f0
    for _ in range(cs.spin_up if spin_up is None else spin_up):
        f = flow_step(streamed(f, cs.fl), cs.fl)
    g = init(cs.c0)
    om = omega_s(cs.D)
    seen = {}
    for n in range(1, (cs.steps if steps is None else steps) + 1):
        f, g = advance(f, g, cs.fl, om, cs.wall, cs.inlet)
        if n in cs.samples:
            seen[n] = field(g, cs.ob)
    return f, seen, field(g, cs.ob)


def probe(c):
    """three numbers that pin a field down: its sum, the sum of its squares and one cell in the middle"""
    return [float(np.sum(c)), float(np.sum(c * c)), float(c[c.shape[0] // 2, c.shape[1] // 3])]


def figures(kind, cs, seen):
    """the figures of a run from its sampled fields (the GPU tests hand in the device's fields)"""
    if kind == "conservation":
        first = total(cs.c0, cs.ob)
        return {"drift": max(abs(total(c, cs.ob) / first - 1.0) for c in seen.values())}
    if kind == "diffusion":
        times = [0] + sorted(seen)
        amps = [diffusion_amplitude(cs.c0)] + [diffusion_amplitude(seen[t]) for t in sorted(seen)]
        rate = diffusion_rate(times, amps)
        return {"rate": rate, "error": rate / diffusion_theory(cs.D) - 1.0}
    if kind == "walls":
        return {"deviation": walls_figure(seen[cs.steps])}
    if kind == "open":
        return {"deviation": float(np.max(np.abs(seen[cs.steps] - 1.0)))}
    ratio, speed = taylor_figures(seen[TAYLOR["t0"]], seen[TAYLOR["t1"]])
    return {"d_eff_ratio": ratio, "speed_ratio": speed}


RUNS = ([("conservation", None)] + [("diffusion", D) for D in DIFFUSION["Ds"]] + [("walls", D) for D in WALLS["Ds"]] +
        [("open", D) for D in OPEN["Ds"]] + [("taylor", None)])


def gates(kind, fig, stored=None):
    """the issue's gates on the figures of one run; stored: the fixture's entry, for the conservation gate's rule"""
    if kind == "conservation":
        gate = CONSERVATION["gate"]
        if stored is not None and stored["drift"] > 1e-13:
            gate = 10.0 * stored["drift"]          # the restatement's own value decides, where it exceeds 1e-13
        assert fig["drift"] <= gate, fig
    elif kind == "diffusion":
        assert abs(fig["error"]) <= DIFFUSION["gate"], fig
    elif kind == "walls":
        assert fig["deviation"] <= WALLS["gate"], fig
    elif kind == "open":
        assert fig["deviation"] <= OPEN["gate"], fig
    else:
        assert abs(fig["d_eff_ratio"] - 1.0) <= TAYLOR["gate"], fig
        assert abs(fig["speed_ratio"] - 1.0) <= TAYLOR["speed_gate"], fig
