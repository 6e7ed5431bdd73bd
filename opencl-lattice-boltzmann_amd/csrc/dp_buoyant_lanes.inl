// The lane body of d2q9_dp_buoyant and d2q9_dp_buoyant_gated (dp_buoyant_kernels.h), included as text inside each kernel, behind
// the kernel's argument `const DpBuoyArgs a` and its flags FORCE, TRT, OPEN, WALL, LES.  Text and not a __device__ function: a body
// inlined from a function comes out of the compiler scheduled otherwise (tools/dp_isa_diff.py), and the 32 instances of
// d2q9_dp_buoyant are to stay the instructions of a library without the gated form.
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  const unsigned lpr = (unsigned)a.lanes_per_row;
  const size_t member = blockIdx.y;
  const int y = (int)(t / lpr);
  const int x0 = 2 * (int)(t - (unsigned)y * lpr);
  const size_t cells = (size_t)a.nx * a.ny;
  double tot = 0.0;
  double tfx = 0.0, tfy = 0.0;
  const bool live = y < a.ny && x0 < a.nx;
  if (live) {
    const DpBuoyMember mc = a.members[member];
    const bool has_b = x0 + 1 < a.nx;
    const size_t ps = a.plane_stride, rs = 9 * ps, gs = 5 * ps;
    const int ys = (y == 0) ? a.ny - 1 : y - 1, yn = (y + 1 == a.ny) ? 0 : y + 1;  // kernels.cl:91-93
    const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;                                  // kernels.cl:99-102
    const int xe = (x0 + 2 < a.nx) ? x0 + 2 : 0;  // east of cell x0+1, or of x0 when x0 is the row's last cell
    const double *src = a.src + member * a.member_stride;
    const double *rc = src + (size_t)y * rs, *rsth = src + (size_t)ys * rs, *rnth = src + (size_t)yn * rs;
    const v2d c0 = *reinterpret_cast<const v2d *>(rc + x0);
    const v2d c1 = *reinterpret_cast<const v2d *>(rc + ps + x0);
    const v2d c3 = *reinterpret_cast<const v2d *>(rc + 3 * ps + x0);
    const v2d c2 = *reinterpret_cast<const v2d *>(rsth + 2 * ps + x0);
    const v2d c5 = *reinterpret_cast<const v2d *>(rsth + 5 * ps + x0);
    const v2d c6 = *reinterpret_cast<const v2d *>(rsth + 6 * ps + x0);
    const v2d c4 = *reinterpret_cast<const v2d *>(rnth + 4 * ps + x0);
    const v2d c7 = *reinterpret_cast<const v2d *>(rnth + 7 * ps + x0);
    const v2d c8 = *reinterpret_cast<const v2d *>(rnth + 8 * ps + x0);
    const double w1 = rc[ps + xw], w5 = rsth[5 * ps + xw], w8 = rnth[8 * ps + xw];
    const double e3 = rc[3 * ps + xe], e6 = rsth[6 * ps + xe], e7 = rnth[7 * ps + xe];
    // the two cells' own five scalar values
    const double *sc = a.scalar + member * (gs * (size_t)a.ny) + (size_t)y * gs + x0;
    v2d s[5];
#pragma unroll
    for (int k = 0; k < 5; k++) s[k] = *reinterpret_cast<const v2d *>(sc + k * ps);
    const uint8_t *mask = a.mask + member * cells;
    const uint8_t *m = mask + (size_t)y * a.nx + x0;
    const bool ob_a = m[0] != 0, ob_b = has_b && m[1] != 0;
    double ga[9] = {c0.x, w1, c2.x, has_b ? c3.y : e3, c4.x, w5, has_b ? c6.y : e6, has_b ? c7.y : e7, w8};
    double gb[9] = {c0.y, c1.x, c2.y, e3, c4.y, c5.x, e6, e7, c8.x};
    if constexpr (FORCE) {
      double fxa = 0.0, fya = 0.0, fxb = 0.0, fyb = 0.0;
      // cell x of this row: its own planes 1..8 and the masks of (x -+ 1, y -+ 1), periodic (kernels.cl:91-102)
      auto cell_force = [&](int x, const double (&g)[9], double &fx, double &fy) {
        const int xl = (x == 0) ? a.nx - 1 : x - 1, xr = (x + 1 == a.nx) ? 0 : x + 1;
        const uint8_t *mr = mask + (size_t)y * a.nx, *ms = mask + (size_t)ys * a.nx, *mn = mask + (size_t)yn * a.nx;
        double own[9];
        own[0] = 0.0;
#pragma unroll
        for (int k = 1; k < 9; k++) own[k] = rc[k * ps + x];
        const uint8_t nb[9] = {0, mr[xl], ms[x], mr[xr], mn[x], ms[xl], ms[xr], mn[xr], mn[xl]};
        dp_force_cell(g, own, nb, fx, fy);
      };
      // byte 1: blocked and counted; 2: blocked, outside the body (include/lbm.h, "Drag of a body")
      if (m[0] == 1) cell_force(x0, ga, fxa, fya);
      if (has_b && m[1] == 1) cell_force(x0 + 1, gb, fxb, fyb);
      tfx = has_b ? fxa + fxb : fxa + 0.0;
      tfy = has_b ? fya + fyb : fya + 0.0;
    }
    if constexpr (OPEN) {
      if (x0 == 0 && !ob_a) dp_open_inlet(ga, mc.u_in[y]);
      if (has_b) {
        if (x0 + 2 == a.nx && !ob_b) dp_open_outlet(gb, mc.rho_out);
      } else if (!ob_a) {
        dp_open_outlet(ga, mc.rho_out);   // nx odd: the row's last lane holds column nx - 1 alone
      }
    }
    const double sa[5] = {s[0].x, s[1].x, s[2].x, s[3].x, s[4].x}, sb[5] = {s[0].y, s[1].y, s[2].y, s[3].y, s[4].y};
    const DpDriveCell drv_a{dp_buoy_force(sa, mc.buoy)}, drv_b{dp_buoy_force(sb, mc.buoy)};
    double oa[9], ob[9];
    const double ta = dp_collide_cell<TRT, LES, true, DpDriveCell>(ga, ob_a, mc.omega, mc.omega_m, mc.les, drv_a, oa);
    const double tb = dp_collide_cell<TRT, LES, true, DpDriveCell>(gb, ob_b, mc.omega, mc.omega_m, mc.les, drv_b, ob);
    if constexpr (WALL) {
      const double *wu_x = a.wall_u + member * cells, *wu_y = a.wall_u + ((size_t)gridDim.y + member) * cells;
      const size_t at = (size_t)y * a.nx + x0;   // ob_b implies has_b: at + 1 is a cell of this row
      if (ob_a) {
        const double u_x = wu_x[at], u_y = wu_y[at];
        if (dp_wall_moves(u_x, u_y)) dp_wall_cell(oa, u_x, u_y, mc.rho_wall);
      }
      if (ob_b) {
        const double u_x = wu_x[at + 1], u_y = wu_y[at + 1];
        if (dp_wall_moves(u_x, u_y)) dp_wall_cell(ob, u_x, u_y, mc.rho_wall);
      }
    }
    if (y == a.accel_row) {
      dp_accelerate_cell(oa, ob_a, mc.aw1, mc.aw2);
      dp_accelerate_cell(ob, ob_b, mc.aw1, mc.aw2);
    }
    double *d = a.dst + member * a.member_stride + (size_t)y * rs + x0;
    if (has_b) {
#pragma unroll
      for (int k = 0; k < 9; k++) {
        v2d v = {oa[k], ob[k]};
        *reinterpret_cast<v2d *>(d + k * ps) = v;
      }
      tot = ta + tb;
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) d[k * ps] = oa[k];
      tot = ta + 0.0;
    }
  }
  // the segment's tree across its eight lanes, written at the member's place: [members][ny][nseg] per value
  const unsigned nseg = lpr >> 3, lane = t - (unsigned)y * lpr;
  const size_t per = (size_t)a.ny * nseg, at = member * per + (size_t)y * nseg + (lane >> 3);
  tot = dp_segment_tree8(tot);
  if (y < a.ny && (lane & 7u) == 0) a.seg[at] = tot;
  if constexpr (FORCE) {
    tfx = dp_segment_tree8(tfx);
    tfy = dp_segment_tree8(tfy);
    if (y < a.ny && (lane & 7u) == 0) {
      const size_t comp = (size_t)gridDim.y * per;
      a.seg[comp + at] = tfx;
      a.seg[2 * comp + at] = tfy;
    }
  }
