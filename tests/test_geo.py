"""Row N3: batched WGS84 <-> ENU.  The oracle (oracle/geo_oracle.c) is PINNED by the reference's own
README output (readme.md:10-28, 15 decimals), committed as tests/golden/G1_readme_geo.json."""
import json
import os

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "G1_readme_geo.json")))
    lla = np.array(g["wgs84_lon_lat_alt"], dtype=float)
    ref = lla[0].copy()
    ref[2] = 0.0   # origin altitude forced to 0 (uavPathPlanning.cpp:3643-3644)
    return lla, ref, np.array(g["enu_east_north_up"], dtype=float), np.array(g["wgs84_round_trip_lon_lat_alt"], dtype=float)


def test_oracle_reproduces_the_readme():
    lla, ref, enu_gold, back_gold = _golden()
    enu = oracle.wgs84_to_enu(lla, ref)
    assert np.max(np.abs(enu - enu_gold)) < 5e-12          # printed with 15 decimals on 2e4-m values
    back = oracle.enu_to_wgs84(enu, ref)
    assert np.max(np.abs(back[:, :2] - back_gold[:, :2])) < 1e-14
    assert np.max(np.abs(back[:, 2] - back_gold[:, 2])) < 1e-9


@pytest.mark.gpu
def test_hip_reproduces_the_readme_and_the_oracle(csp):
    lla, ref, enu_gold, back_gold = _golden()
    enu = csp.wgs84_to_enu_batch(lla, ref)
    assert np.max(np.abs(enu - enu_gold)) < 1e-8           # metres; device libm differs in the last ulps
    back = csp.enu_to_wgs84_batch(enu, ref)
    assert np.max(np.abs(back[:, :2] - back_gold[:, :2])) < 1e-12
    assert np.max(np.abs(back[:, 2] - back_gold[:, 2])) < 1e-8
    rng = np.random.default_rng(3)
    n = 200000
    pts = np.stack([rng.uniform(-180, 180, n), rng.uniform(-89.9, 89.9, n), rng.uniform(-500, 12000, n)], axis=1)
    ref2 = np.array([109.56, 40.87, 0.0])
    e_gpu, e_cpu = csp.wgs84_to_enu_batch(pts, ref2), oracle.wgs84_to_enu(pts, ref2)
    assert np.max(np.abs(e_gpu - e_cpu)) < 1e-7            # on values up to 1.3e7 m: 1e-14 relative
    near = np.stack([rng.uniform(-5e4, 5e4, n), rng.uniform(-5e4, 5e4, n), rng.uniform(0, 5e3, n)], axis=1)
    l_gpu, l_cpu = csp.enu_to_wgs84_batch(near, ref2), oracle.enu_to_wgs84(near, ref2)
    assert np.max(np.abs(l_gpu[:, :2] - l_cpu[:, :2])) < 1e-12
    assert np.max(np.abs(l_gpu[:, 2] - l_cpu[:, 2])) < 1e-7
    # round trip on the device
    import torch
    d = torch.from_numpy(near).cuda()
    rt = csp.wgs84_to_enu_batch(csp.enu_to_wgs84_batch(d, ref2), ref2).cpu().numpy()
    assert np.max(np.abs(rt - near)) < 1e-6


def _mp_round_trip(bits=None):
    from tests import geo_ref
    lla, ref, enu_gold, back_gold = _golden()
    enu = geo_ref.wgs84_to_enu(lla, ref, bits=bits)
    return lla, ref, enu, enu_gold, geo_ref.enu_to_wgs84(enu, ref, bits=bits), back_gold


def test_mpmath_reference_reproduces_the_readme():
    """tests/geo_ref.py at the gates of test_oracle_reproduces_the_readme.  The README's numbers are the output of an fp64
    evaluation, so the module is evaluated here with every operation rounded to 53 bits (its precision is a parameter; the
    formulas and their order are the ones it uses at 50 digits): it then reproduces the README inside the file's gates
    and the C oracle to a few ulps (4 ulp of an ECEF coordinate, 6.4e6 m, for metres; 4 ulp of 180 for degrees: on this
    fixture the two agree bit for bit when the host libm rounds sin, cos, atan2 and sqrt correctly, as mpmath does, and
    a libm that is one ulp off in some call moves a result by about as much), which pins the restatement operation
    for operation."""
    lla, ref, enu, enu_gold, back, back_gold = _mp_round_trip(bits=53)
    print("geo_ref at 53 bits against the README: ENU %.3e m, lon/lat %.3e deg, alt %.3e m" % (
        np.max(np.abs(enu - enu_gold)), np.max(np.abs(back[:, :2] - back_gold[:, :2])), np.max(np.abs(back[:, 2] - back_gold[:, 2]))))
    assert np.max(np.abs(enu - enu_gold)) < 5e-12
    assert np.max(np.abs(back[:, :2] - back_gold[:, :2])) < 1e-14
    assert np.max(np.abs(back[:, 2] - back_gold[:, 2])) < 1e-9
    back_or = oracle.enu_to_wgs84(enu, ref)
    assert np.max(np.abs(enu - oracle.wgs84_to_enu(lla, ref))) <= 4 * np.spacing(6.4e6)
    assert np.max(np.abs(back[:, :2] - back_or[:, :2])) <= 4 * np.spacing(180.0)
    assert np.max(np.abs(back[:, 2] - back_or[:, 2])) <= 4 * np.spacing(6.4e6)


def test_mpmath_reference_is_within_fp64_rounding_of_the_readme():
    """The same module at its 50 digits, as the GPU tests use it: the README, being fp64 output, sits 1.61e-9 m,
    1.42e-14 degrees and 8.6e-10 m from it, inside what the number format allows.  ENU: each ECEF coordinate of the point
    and of the origin (up to 6.4e6 m, ulp 9.3e-10 m) carries about three roundings (N, two trigonometric products) and
    the rotation adds one: 8 ulp = 7.5e-9 m.  Longitude / latitude: atan2, the product with 180 and the division by pi
    on values near 110 degrees (ulp 1.42e-14): 4 ulp = 5.7e-14.  Altitude: the file's own 1e-9 m."""
    _, _, enu, enu_gold, back, back_gold = _mp_round_trip()
    assert np.max(np.abs(enu - enu_gold)) < 8 * np.spacing(6.4e6)
    assert np.max(np.abs(back[:, :2] - back_gold[:, :2])) < 4 * np.spacing(110.0)
    assert np.max(np.abs(back[:, 2] - back_gold[:, 2])) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# Both kernels against tests/geo_ref.py (mpmath) away from latitude 40.87: the equator, mid latitudes, 1 degree and
# 0.01 degree (1.1 km) from either pole, and reference longitudes 0.1 degree from the antimeridian on either side.
# EXCLUDED from the gates: the exact pole (p = 0: the longitude is undefined and the altitude takes the reference's
# special branch) and points exactly on the +-180 degree cut (atan2's sign there depends on the sign of a zero).  The
# random points below never hit either.
#
# Gate, per reference point and per quantity (ENU metres; longitude, latitude degrees; altitude metres), with e(x) the
# largest absolute difference from geo_ref over the reference point's 64 targets:  e_kernel <= K_GEO * e_oracle + floor.
# The floors are 4 ulps of the largest intermediate: 6.4e6 m (ECEF) for metres, 180 for degrees.  K_GEO = 8 is picked
# from the ratios measured on an MI355X with more than 2x headroom:
#     |lat| of the reference     ENU      longitude   latitude   altitude      altitude error, kernel / oracle [m]
#      0                         1.00     2.00        2.00       1.00          2.3e-09 / 2.3e-09
#     45                         1.10     2.00        2.00       1.32          2.1e-09 / 2.0e-09
#     89                         1.50     1.00        1.00       1.77          9.8e-08 / 6.0e-08
#     89.99                      1.00     1.00        2.00       2.21          1.6e-06 / 7.1e-07
# (worst e_kernel / e_oracle over the three reference longitudes; the ratios of 2.00 are one ulp against two.)  The
# altitude p / cos(lat) - N loses digits like 1 / cos(lat), in the oracle as in the kernel.
REF_LATS = (0.0, 45.0, -45.0, 89.0, -89.0, 89.99, -89.99)
REF_LONS = (0.0, 179.9, -179.9)
K_GEO = 8.0
FLOOR_M, FLOOR_DEG = 4 * np.spacing(6.4e6), 4 * np.spacing(180.0)
PER_REF = 64


def _wrap(lon):
    return (lon + 180.0) % 360.0 - 180.0


def _geo_cases():
    """[(ref, lla targets [64,3], enu targets [64,3])]: forward targets within half a degree of the reference (across the
    antimeridian for the references next to it, clipped 1e-3 degree short of the poles) plus a quarter of them anywhere
    on the globe, altitudes -500 .. 12000 m; inverse targets within 50 km of the reference, up 0 .. 5 km."""
    rng = np.random.default_rng(2024)
    out = []
    for lat0 in REF_LATS:
        for lon0 in REF_LONS:
            ref = np.array([lon0, lat0, 0.0])
            lon = _wrap(lon0 + rng.uniform(-0.5, 0.5, PER_REF))
            lat = np.clip(lat0 + rng.uniform(-0.5, 0.5, PER_REF), -89.999, 89.999)
            far = slice(0, PER_REF // 4)
            lon[far], lat[far] = rng.uniform(-179.999, 179.999, PER_REF // 4), rng.uniform(-89.9, 89.9, PER_REF // 4)
            lla = np.stack([lon, lat, rng.uniform(-500.0, 12000.0, PER_REF)], axis=1)
            enu = np.stack([rng.uniform(-5e4, 5e4, PER_REF), rng.uniform(-5e4, 5e4, PER_REF), rng.uniform(0.0, 5e3, PER_REF)], axis=1)
            assert (np.abs(lla[:, 0]) < 180.0).all()
            out.append((ref, lla, enu))
    return out


_GEO_REFERENCE = []


def _geo_reference():
    """_geo_cases with geo_ref's and the C oracle's results, computed once."""
    from tests import geo_ref
    if not _GEO_REFERENCE:
        for ref, lla, enu in _geo_cases():
            _GEO_REFERENCE.append((ref, lla, enu, geo_ref.wgs84_to_enu(lla, ref), oracle.wgs84_to_enu(lla, ref),
                                   geo_ref.enu_to_wgs84(enu, ref), oracle.enu_to_wgs84(enu, ref)))
    return _GEO_REFERENCE


def _lon_diff(a, b):
    return np.abs(_wrap(a - b))


@pytest.mark.gpu
def test_hip_against_mpmath_over_latitudes_and_the_antimeridian(csp):
    """See the comment above: 21 reference points x 64 targets, forward and inverse, every quantity gated per reference
    point at K_GEO * e_oracle + floor against tests/geo_ref.py; the inverse's altitude error p / cos(lat) - N grows like
    1 / cos(lat) and is reported per latitude band.  Host- and device-memory forms are bit-equal."""
    import torch
    band = {}
    for ref, lla, enu, f_mp, f_or, i_mp, i_or in _geo_reference():
        f_gpu, i_gpu = csp.wgs84_to_enu_batch(lla, ref), csp.enu_to_wgs84_batch(enu, ref)
        f_dev = csp.wgs84_to_enu_batch(torch.from_numpy(lla).cuda(), ref).cpu().numpy()
        i_dev = csp.enu_to_wgs84_batch(torch.from_numpy(enu).cuda(), ref).cpu().numpy()
        assert f_gpu.tobytes() == f_dev.tobytes() and i_gpu.tobytes() == i_dev.tobytes(), ref
        rows = [("enu m", np.abs(f_gpu - f_mp).max(), np.abs(f_or - f_mp).max(), FLOOR_M),
                ("lon deg", _lon_diff(i_gpu[:, 0], i_mp[:, 0]).max(), _lon_diff(i_or[:, 0], i_mp[:, 0]).max(), FLOOR_DEG),
                ("lat deg", np.abs(i_gpu[:, 1] - i_mp[:, 1]).max(), np.abs(i_or[:, 1] - i_mp[:, 1]).max(), FLOOR_DEG),
                ("alt m", np.abs(i_gpu[:, 2] - i_mp[:, 2]).max(), np.abs(i_or[:, 2] - i_mp[:, 2]).max(), FLOOR_M)]
        for name, e_k, e_o, floor in rows:
            print("ref lon %7.1f lat %6.2f  %-7s e_oracle %.3e  e_kernel %.3e  ratio %.2f" % (ref[0], ref[1], name, e_o, e_k, e_k / e_o if e_o else 0.0))
            assert e_k <= K_GEO * e_o + floor, (tuple(ref), name, e_k, e_o)
        b = band.setdefault(abs(ref[1]), [0.0, 0.0])
        b[0], b[1] = max(b[0], rows[3][1]), max(b[1], rows[3][2])
    for lat in sorted(band):
        print("inverse altitude error at |lat| = %5.2f: kernel %.3e m, oracle %.3e m" % (lat, band[lat][0], band[lat][1]))


def _geo_raw(csp, fn, pts, ref, fill):
    """One device-memory call through raw pointers with input and output in guarded carves of exactly n * 24 bytes, the
    output starting as `fill` bytes: return code 0, no guard byte and no input byte changed.  Returns the output."""
    import ctypes
    import torch
    from tests.staged import Carved, check_carves
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    g_in, g_out = Carved(pts, "cuda:0", "in"), Carved(np.zeros_like(pts), "cuda:0", "out", fill)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(csp.raw_lib(), fn)(g_in.data_ptr(), ref.ctypes.data, g_out.data_ptr(), len(pts), csp.MEM_DEVICE, -1, stream)
    assert rc == 0, (fn, rc)
    torch.cuda.synchronize()
    check_carves((fn, len(pts)), [g_in, g_out], [g_in])
    return g_out.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_hip_block_edges_guard_bands_and_a_nan_lane(csp, n):
    """Batches around the 256-thread block with guard-banded input and output (64 KiB of 0xA5 on either side: a lane
    past n would write 24 bytes right behind the output): no guard or input byte changes, every output element is
    written (none keeps the 0xFF fill), and the result is bit-equal with the binding's host-memory call.  n = 0 returns
    CSP_OK and touches nothing.  With a NaN in one lane's input (lane n // 2) every other lane stays bit-equal."""
    rng = np.random.default_rng(n)
    ref = np.array([179.9, -45.0, 0.0])
    lla = np.stack([_wrap(179.9 + rng.uniform(-0.5, 0.5, n)), rng.uniform(-45.5, -44.5, n), rng.uniform(-500, 12000, n)], axis=1)
    enu = np.stack([rng.uniform(-5e4, 5e4, n), rng.uniform(-5e4, 5e4, n), rng.uniform(0, 5e3, n)], axis=1)
    for fn, host, pts in (("csp_geo_wgs84_to_enu_batch", csp.wgs84_to_enu_batch, lla), ("csp_geo_enu_to_wgs84_batch", csp.enu_to_wgs84_batch, enu)):
        got = _geo_raw(csp, fn, pts, ref, 0xFF)
        if n == 0:
            assert got.size == 0
            continue
        assert np.isfinite(got).all() and got.tobytes() == host(pts, ref).tobytes(), (fn, n)
        bad = pts.copy()
        bad[n // 2, 1] = np.nan
        got_bad = _geo_raw(csp, fn, bad, ref, 0xFF)
        keep = np.arange(n) != n // 2
        assert got_bad[keep].tobytes() == got[keep].tobytes(), (fn, n)
        assert np.isnan(got_bad[n // 2]).any(), (fn, n)
