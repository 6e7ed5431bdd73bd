// The lane body of dp_scalar_step and dp_scalar_step_rec (dp_scalar_kernels.h), included as text inside each kernel, behind the
// kernel's argument `a`, the lane's row y and first column x0, and the flags BUOY and RECORD.  RECORD (include/lbm.h, "Scalar
// record"): the lane's pair sums of c, c u_x and c u_y of its fluid cells into `double rec[3]`, from the values the step holds
// anyway: c is dp_scalar_collide's own sum of h, the products are those under its a_x and a_y; a blocked cell adds +0.0.  Text and
// not a __device__ function: a body inlined from a function comes out of the compiler scheduled otherwise (tools/dp_isa_diff.py),
// and dp_scalar_step<false> and <true> are to stay the instructions of a library without the record.
  const DpScalarMember mc = a.members[blockIdx.y];
  const bool has_b = x0 + 1 < a.nx;
  const size_t ps = a.plane_stride, frs = 9 * ps, grs = 5 * ps;
  const int ys = (y == 0) ? a.ny - 1 : y - 1, yn = (y + 1 == a.ny) ? 0 : y + 1;
  const int xw = (x0 == 0) ? a.nx - 1 : x0 - 1;
  const int xe = (x0 + 2 < a.nx) ? x0 + 2 : 0;  // east of cell x0+1, or of x0 when x0 is the row's last cell
  const double *fc = a.flow + mc.flow_off + (size_t)y * frs + x0;
  const double *gc = a.src + mc.state_off + (size_t)y * grs;
  const double *gs = a.src + mc.state_off + (size_t)ys * grs, *gn = a.src + mc.state_off + (size_t)yn * grs;
  v2d f[9];
#pragma unroll
  for (int k = 0; k < 9; k++) f[k] = *reinterpret_cast<const v2d *>(fc + k * ps);
  const v2d c0 = *reinterpret_cast<const v2d *>(gc + x0);
  const v2d c1 = *reinterpret_cast<const v2d *>(gc + ps + x0);
  const v2d c3 = *reinterpret_cast<const v2d *>(gc + 3 * ps + x0);
  const v2d c2 = *reinterpret_cast<const v2d *>(gs + 2 * ps + x0);
  const v2d c4 = *reinterpret_cast<const v2d *>(gn + 4 * ps + x0);
  const double w1 = gc[ps + xw], e3 = gc[3 * ps + xe];
  const uint8_t *mask = a.mask + mc.cell_off;
  const uint8_t *mrow = mask + (size_t)y * a.nx, *msth = mask + (size_t)ys * a.nx, *mnth = mask + (size_t)yn * a.nx;
  const double *cw = a.c_wall + mc.cell_off;
  const bool ob_a = mrow[x0] != 0, ob_b = has_b && mrow[x0 + 1] != 0;
  const bool blk_w = mrow[xw] != 0, blk_e = mrow[xe] != 0;

  // cell x of this row: own = its stored g_0, g_1, g_3; east / west: the streamed values and whether their cells are blocked
  auto cell = [&](int x, bool blocked, double own0, double own1, double own3, double from_w, bool w_blocked, int x_w, double from_e,
                  bool e_blocked, int x_e, double from_s, double from_n, const double (&fl)[9], const double *drv, double (&out)[5],
                  double (&sum)[3]) {
    if (blocked) {
      out[0] = own0; out[1] = own1; out[2] = gc[2 * ps + x]; out[3] = own3; out[4] = gc[4 * ps + x];
      if constexpr (RECORD) sum[0] = sum[1] = sum[2] = 0.0;
      return;
    }
    double h[5];
    h[0] = own0;
    h[1] = w_blocked ? dp_scalar_wall(own3, cw[(size_t)y * a.nx + x_w]) : from_w;
    h[3] = e_blocked ? dp_scalar_wall(own1, cw[(size_t)y * a.nx + x_e]) : from_e;
    h[2] = from_s;
    if (msth[x] != 0) h[2] = dp_scalar_wall(gc[4 * ps + x], cw[(size_t)ys * a.nx + x]);
    h[4] = from_n;
    if (mnth[x] != 0) h[4] = dp_scalar_wall(gc[2 * ps + x], cw[(size_t)yn * a.nx + x]);
    if (a.open) {
      if (x == 0) h[1] = a.c_in[mc.in_off + y] - (((h[0] + h[2]) + h[3]) + h[4]);
      if (x == a.nx - 1) h[3] = own3;
    }
    double u_x, u_y, uu, pr;
    dp_output_cell(fl, drv, u_x, u_y, uu, pr);
    dp_scalar_collide(h, u_x, u_y, mc.omega_s, out);
    if constexpr (RECORD) {
      const double c = (((h[0] + h[1]) + h[2]) + h[3]) + h[4];
      sum[0] = c;
      sum[1] = c * u_x;
      sum[2] = c * u_y;
    }
  };

  double fa[9], fb[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    fa[k] = f[k].x;
    fb[k] = f[k].y;
  }
  double oa[5], ob[5];
  [[maybe_unused]] double ra[3], rb[3];
  // the force of each cell's own five stored values; without BUOY the member's body force, or NULL
  [[maybe_unused]] double pa[2], pb[2];
  const double *drv_a = mc.drive, *drv_b = mc.drive;
  if constexpr (BUOY) {
    const DpBuoy bu = a.buoy[blockIdx.y].buoy;
    const v2d o2 = *reinterpret_cast<const v2d *>(gc + 2 * ps + x0);
    const v2d o4 = *reinterpret_cast<const v2d *>(gc + 4 * ps + x0);
    const double sa[5] = {c0.x, c1.x, o2.x, c3.x, o4.x}, sb[5] = {c0.y, c1.y, o2.y, c3.y, o4.y};
    const DpDrive fa_ = dp_buoy_force(sa, bu), fb_ = dp_buoy_force(sb, bu);
    pa[0] = fa_.f_x, pa[1] = fa_.f_y;
    pb[0] = fb_.f_x, pb[1] = fb_.f_y;
    drv_a = pa, drv_b = pb;
  }
  // cell a: its west neighbour is column xw, its east neighbour cell b or, where the lane has none, column xe
  cell(x0, ob_a, c0.x, c1.x, c3.x, w1, blk_w, xw, has_b ? c3.y : e3, has_b ? ob_b : blk_e, has_b ? x0 + 1 : xe, c2.x, c4.x, fa, drv_a, oa,
       ra);
  double *d = a.dst + mc.state_off + (size_t)y * grs + x0;
  if (has_b) {
    cell(x0 + 1, ob_b, c0.y, c1.y, c3.y, c1.x, ob_a, x0, e3, blk_e, xe, c2.y, c4.y, fb, drv_b, ob, rb);
#pragma unroll
    for (int k = 0; k < 5; k++) {
      v2d v = {oa[k], ob[k]};
      *reinterpret_cast<v2d *>(d + k * ps) = v;
    }
    if constexpr (RECORD) {
#pragma unroll
      for (int v = 0; v < 3; v++) rec[v] = ra[v] + rb[v];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) d[k * ps] = oa[k];
    if constexpr (RECORD) {
#pragma unroll
      for (int v = 0; v < 3; v++) rec[v] = ra[v] + 0.0;
    }
  }
