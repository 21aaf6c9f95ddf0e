"""
GPU: csrc/draw.hip (gpp_draw_build, gpp_draw_raster) against tests/draw_oracle.py, and the composites of
RetinaNet3D.predict_composites_on_frames / bin/run_network.py --device-pose --save-images against the host renderer
(utils/visualization.py) -- DESIGN.md section 4.14.

Bars.  The rasteriser is integer arithmetic: tolerance zero, every byte.  The build stage is float64 with its own sine and cosine, the
oracle uses math.sin / math.cos: a truncated endpoint may differ by exactly one where the oracle's real-valued coordinate lies within 1e-6
of an integer (expected share of endpoints about 2e-6; such excuses are capped at 0.1 %), every other field is identical.  The end-to-end
tests first assert that none of their own inputs has a projected coordinate that close to an integer, so no excuse applies to them.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import draw_oracle
from test_draw_cpu import P_KITTI, frame_of, random_rows
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import synthetic
from keras_retinanet_3D.utils import visualization as vis
from keras_retinanet_3D.utils.image import compute_resize_scale

pytestmark = pytest.mark.gpu

POISON = 0xA5
KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]


def device():
    return torch.device('cuda', torch.cuda.current_device())


def raster_on_device(frames, tables, Hr=None, Wr=None):
    """ frames: a list of (h, w, 3) uint8; tables: per image an (n, 16) int32 array -> (the composites, the poisoned slots as the raster left them, status) """
    dev = device()
    B = len(frames)
    Hr = Hr or max(f.shape[0] for f in frames)
    Wr = Wr or max(f.shape[1] for f in frames)
    cap = max(max(len(t) for t in tables), 1)
    raw = np.zeros((B, Hr * Wr * 3), np.uint8)
    prims = np.zeros((B, cap, 16), np.int32)
    counts = np.zeros((B, 4), np.int32)
    for b, (f, t) in enumerate(zip(frames, tables)):
        raw[b, :f.size] = f.reshape(-1)
        prims[b, :len(t)] = t
        counts[b] = (0, len(t), b * cap, 0)
    out = torch.full((B, 2 * Hr * Wr * 3), POISON, dtype=torch.uint8, device=dev)
    status = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    hw = torch.as_tensor(np.array([f.shape[:2] for f in frames], np.int32)).to(dev)
    hip.draw_raster(torch.as_tensor(raw).to(dev), hw, Hr, Wr, torch.as_tensor(prims).to(dev), torch.as_tensor(counts).to(dev), out, status)
    slots = out.cpu().numpy()
    pictures = [slots[b, :2 * f.shape[0] * f.shape[1] * 3].reshape(2 * f.shape[0], f.shape[1], 3) for b, f in enumerate(frames)]
    return pictures, slots, status.cpu().numpy()


def fuzzed_table(rng, h, w, n, far):
    """ n records of every kind; coordinates around the frame, now and then far off it """
    def pt():
        reach = [40, 40, 40, 400, far][int(rng.integers(5))]
        return int(rng.integers(-reach, w + reach)), int(rng.integers(-reach, h + reach))
    recs = []
    for _ in range(n):
        kind = int(rng.integers(1, 6))
        picture = int(rng.integers(2))
        color = tuple(int(c) for c in rng.integers(0, 256, 3))
        p, q = pt(), pt()
        if rng.integers(10) == 0:
            q = p
        if kind == vis.KIND_LINE:
            recs.append(vis.line_record(picture, p, q, color))
        elif kind == vis.KIND_DASHED:
            recs.append(vis.line_record(picture, p, q, color, dashed=True))
        elif kind == vis.KIND_RECT:
            recs.append(vis.rect_record(picture, p[0], p[1], q[0], q[1], color))
        elif kind == vis.KIND_CIRCLE:
            recs.append(vis.circle_record(picture, p[0], p[1], color))
        else:
            text = ''.join(vis.GLYPH_CHARS[int(i)] for i in rng.integers(0, len(vis.GLYPH_CHARS), int(rng.integers(0, vis.CAPTION_MAX + 1))))
            recs.append(vis.caption_record(picture, p[0], p[1], text))
        if rng.integers(12) == 0:
            recs.append(np.zeros(16, np.int32))                       # an empty slot
    return np.stack(recs).astype(np.int32)


@pytest.mark.parametrize('seed,sizes,n,far', [
    (0, [(37, 150), (40, 131), (21, 64), (40, 150)], 60, 3000),           # ragged sizes in one batch
    (1, [(64, 200)], 700, 3000),                                         # more records than one pass of a workgroup examines
    (2, [(50, 70), (49, 67)], 25, 1000000),                              # endpoints at the edge of the coordinate range
    (3, [(33, 129), (33, 129), (33, 129)], 8, 200),                      # a uniform batch, sparse: most tiles are plain copies
])
def test_raster_matches_the_oracle_byte_for_byte(seed, sizes, n, far):
    rng = np.random.default_rng(seed)
    frames = [frame_of(rng, h, w) for h, w in sizes]
    tables = [fuzzed_table(rng, h, w, n, far) for h, w in sizes]
    pictures, slots, status = raster_on_device(frames, tables)
    for b, (f, t) in enumerate(zip(frames, tables)):
        want = draw_oracle.rasterise(f, t.tolist())
        assert np.array_equal(pictures[b], want), 'image {}: {} bytes differ'.format(b, int((pictures[b] != want).sum()))
        assert np.array_equal(vis.raster(f, t), want)
        assert (slots[b, want.size:] == POISON).all(), 'image {}: bytes beyond its own 2h x w x 3 were written'.format(b)
        assert status[b].tolist() == [len(t), 0, 2 * f.shape[0], f.shape[1]]
    assert any(not np.array_equal(p, np.vstack((f, f))) for p, f in zip(pictures, frames))


def test_raster_in_a_wider_slot_and_with_unknown_records():
    rng = np.random.default_rng(7)
    frames = [frame_of(rng, 30, 90), frame_of(rng, 28, 100)]
    tables = [fuzzed_table(rng, 30, 90, 30, 500), fuzzed_table(rng, 28, 100, 30, 500)]
    tables[1][3, 0] = 9                       # a kind no rule knows: counted, never drawn
    tables[1][5, 1] = 2                       # a picture that does not exist
    pictures, slots, status = raster_on_device(frames, tables, Hr=41, Wr=133)
    known = tables[1].copy()
    known[[3, 5]] = 0
    assert np.array_equal(pictures[0], draw_oracle.rasterise(frames[0], tables[0].tolist()))
    assert np.array_equal(pictures[1], draw_oracle.rasterise(frames[1], known.tolist()))
    assert status[:, 1].tolist() == [0, 2]
    for b, f in enumerate(frames):
        assert (slots[b, 2 * f.size:] == POISON).all()


def check_tables(got, rows, P, thr):
    """ one image's device table against the oracle's; returns (endpoints compared, endpoints excused) """
    reals = []
    n, recs = draw_oracle.build(rows, P, thr, real=reals)
    want = np.asarray(recs, dtype=np.int64).reshape(-1, 16)
    got = got[:len(want)].astype(np.int64)
    endpoints = excused = 0
    for i in np.nonzero((got != want).any(axis=1))[0]:
        assert reals[i] is not None, 'record {} differs and is no cuboid edge: {} != {}'.format(i, got[i].tolist(), want[i].tolist())
        assert np.array_equal(got[i][[0, 1, 6]], want[i][[0, 1, 6]]) and np.array_equal(got[i][11:], want[i][11:])
        for c in range(4):
            if got[i][2 + c] != want[i][2 + c]:
                real = reals[i][c]
                assert abs(got[i][2 + c] - want[i][2 + c]) == 1 and abs(real - round(real)) < 1e-6, (i, c, real, got[i].tolist(), want[i].tolist())
                excused += 1
        g = 1 if got[i][0] == vis.KIND_DASHED else 0
        x0, y0, x1, y1 = got[i][2:6]
        assert got[i][7:11].tolist() == [min(x0, x1) - g, min(y0, y1) - g, max(x0, x1) + g, max(y0, y1) + g]
    endpoints = 4 * sum(r is not None for r in reals)
    return n, endpoints, excused


def test_build_matches_the_oracle_on_ten_thousand_rows():
    rng = np.random.default_rng(11)
    B, D = 8, 1300
    assert B * D >= 10 ** 4
    rows = np.stack([random_rows(rng, D, 375, 1242, spread=[1.0, 1.0, 2.0, 6.0][b % 4]) for b in range(B)])
    for b in range(B):
        rows[b, :, 12] = rng.permutation(rows[b, :, 12])           # no order: the rank of a row is a prefix sum, not its index
    rows[1, 5, 12] = np.nan
    rows[2, 7, 22:25] = np.nan
    rows[3, 9, 19:22] = [0.2, 1.5, 0.5]
    P = np.stack([P_KITTI * [[1.0 + 0.01 * b], [1.0 + 0.01 * b], [1.0]] for b in range(B)])
    dev = device()
    prims, counts = hip.draw_build(torch.as_tensor(rows).to(dev), torch.as_tensor(P).to(dev), 0.4)
    prims, counts = prims.cpu().numpy(), counts.cpu().numpy()
    endpoints = excused = drawn = 0
    for b in range(B):
        n, e, x = check_tables(prims[b], rows[b], P[b], 0.4)
        assert counts[b].tolist() == [n, 26 * n, b * D * 26, 0]
        endpoints, excused, drawn = endpoints + e, excused + x, drawn + n
    print('gpp_draw_build: {} rows drawn, {} cuboid endpoints, {} excused'.format(drawn, endpoints, excused))
    assert drawn > 4000 and endpoints > 10 ** 5
    assert excused <= 1e-3 * endpoints


def test_bad_arguments_and_empty_batches():
    dev = device()
    lib = hip.lib()
    buf = torch.full((4096,), 7, dtype=torch.int32, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 2)
    n_a, n_b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gpp_draw_workspace_bytes(2, 100, ctypes.byref(n_a), ctypes.byref(n_b)) == 0 and (n_a.value, n_b.value) == (2 * 100 * 26 * 64, 2 * 16)
    assert lib.gpp_draw_workspace_bytes(-1, 1, ctypes.byref(n_a), ctypes.byref(n_b)) == -1
    assert lib.gpp_draw_workspace_bytes(1, -1, ctypes.byref(n_a), ctypes.byref(n_b)) == -1
    assert lib.gpp_draw_workspace_bytes(1, 1, None, ctypes.byref(n_b)) == -1 and lib.gpp_draw_workspace_bytes(1, 1, ctypes.byref(n_a), None) == -1
    good = [p, p, 1, 1, 0.4, p, p, None]
    for k, v in ((0, None), (1, None), (5, None), (6, None), (2, -1), (3, -1), (0, odd), (1, odd), (5, odd), (6, odd)):
        a = list(good)
        a[k] = v
        assert lib.gpp_draw_build(*a) == -1, k
    good = [p, p, 4, 4, p, p, 1, p, p, None]
    for k, v in ((0, None), (1, None), (5, None), (7, None), (8, None), (2, -1), (3, -1), (6, -1), (1, odd), (4, odd), (5, odd), (8, odd)):
        a = list(good)
        a[k] = v
        assert lib.gpp_draw_raster(*a) == -1, k
    assert lib.gpp_draw_build(p, p, 0, 5, 0.4, p, p, None) == 0 and lib.gpp_draw_raster(p, p, 4, 4, p, p, 0, p, p, None) == 0
    assert lib.gpp_draw_raster(p, p, 0, 4, p, p, 1, p, p, None) == 0
    torch.cuda.synchronize()
    assert (buf == 7).all()                                          # nothing was launched
    # D == 0: counts of zero, and the raster copies the frames
    rng = np.random.default_rng(3)
    frames = np.stack([frame_of(rng, 19, 70) for _ in range(2)])
    prims, counts = hip.draw_build(torch.zeros((2, 0, 36), dtype=torch.float32, device=dev), torch.as_tensor(np.stack([P_KITTI] * 2)).to(dev), 0.4)
    assert counts.cpu().numpy().tolist() == [[0, 0, 0, 0]] * 2
    out = torch.full((2, 2 * 19 * 70 * 3), POISON, dtype=torch.uint8, device=dev)
    status = torch.zeros((2, 4), dtype=torch.int32, device=dev)
    hip.draw_raster(torch.as_tensor(frames).to(dev), torch.as_tensor(np.array([[19, 70]] * 2, np.int32)).to(dev), 19, 70, prims, counts, out, status)
    got = out.cpu().numpy().reshape(2, 38, 70, 3)
    assert np.array_equal(got, np.concatenate([frames, frames], axis=1))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def posed():
    patch = pytest.MonkeyPatch()
    patch.setenv('GPP_AUTOTUNE', '0')                           # (a tile never changes a byte: tests/test_network_gpu.py)
    yield models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f16x3', pose=True)
    patch.undo()


def noise_frames(shapes, seed):
    """ binary noise keeps the synthetic weights' scores above the 0.05 threshold """
    return [(np.random.default_rng(seed + k).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8) for k, (h, w) in enumerate(shapes)]


def calibrations(shapes, P2):
    scales = [compute_resize_scale((h, w, 3)) for h, w in shapes]
    P_inv = np.stack([np.linalg.pinv(np.diag([s, s, 1.0]).dot(P2)) for s in scales]).astype(np.float32)
    return P_inv, np.stack([P2] * len(shapes))


def no_coordinate_near_an_integer(rows, counts, P_raw, thr):
    for b in range(len(rows)):
        reals = []
        draw_oracle.build(rows[b][:counts[b]], P_raw[b], thr, real=reals)
        for r in reals:
            if r is not None:
                assert all(abs(c - round(c)) >= 1e-6 for c in r), r


def check_composites(posed, frames, P2, thr, n_planes='100'):
    shapes = [f.shape[:2] for f in frames]
    P_inv, P_raw = calibrations(shapes, P2)
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    batch = frames if len(set(shapes)) > 1 else np.stack(frames)
    (before, counts_before), _ = posed.predict_poses_on_frames(batch, P_inv, planes)
    (rows, counts), scale, pictures = posed.predict_composites_on_frames(batch, P_inv, planes, P_raw, thr)
    assert rows.tobytes() == before.tobytes() and counts.tobytes() == counts_before.tobytes()
    no_coordinate_near_an_integer(rows, counts, P_raw, thr)
    assert len(pictures) == len(frames)
    for b, f in enumerate(frames):
        want = vis.composite_from_rows(f, rows[b], counts[b], P_raw[b], thr)
        assert pictures[b].dtype == np.uint8 and pictures[b].shape == (2 * f.shape[0], f.shape[1], 3)
        assert np.array_equal(pictures[b], want), 'image {}: {} bytes differ'.format(b, int((pictures[b] != want).sum()))
    # twice the same bytes; the pose call still returns what it returned
    (_, _), _, again = posed.predict_composites_on_frames(batch, P_inv, planes, P_raw, thr)
    assert all(np.array_equal(a, p) for a, p in zip(again, pictures))
    (after, counts_after), _ = posed.predict_poses_on_frames(batch, P_inv, planes)
    assert after.tobytes() == before.tobytes() and counts_after.tobytes() == counts_before.tobytes()
    # an image alone is the same image inside the batch
    alone_batch = [frames[-1]] if isinstance(batch, list) else batch[-1:]
    (_, _), _, alone = posed.predict_composites_on_frames(alone_batch, P_inv[-1:], planes, P_raw[-1:], thr)
    assert np.array_equal(alone[0], pictures[-1])
    return rows, counts, pictures


@pytest.mark.parametrize('thr', [0.05, 0.4])
def test_composites_at_a_small_shape(posed, thr):
    """ a uniform batch of small raw frames (the network still sees them resized to 800 x 1333) """
    frames = noise_frames([(96, 160)] * 2, seed=96)
    P2 = P_KITTI * [[0.15], [0.15], [1.0]]                      # the principal point inside the small frame
    check_composites(posed, frames, P2, thr)


@pytest.mark.parametrize('thr', [0.05, 0.4])
def test_composites_of_the_four_kitti_sizes_as_one_list(posed, thr):
    frames = noise_frames(KITTI_SHAPES, seed=375)
    rows, counts, pictures = check_composites(posed, frames, synthetic.KITTI_LIKE_P2, thr, n_planes='1k')
    if thr == 0.05:
        assert counts.sum() > 0
        assert any(not np.array_equal(p, np.vstack((f, f))) for p, f in zip(pictures, frames))


def test_a_model_without_a_pose_stage_refuses(posed):
    plain = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f16x3')
    frames = np.stack(noise_frames([(96, 160)], seed=1))
    P_inv, P_raw = calibrations([(96, 160)], P_KITTI)
    with pytest.raises(hip.GppError):
        plain.predict_composites_on_frames(frames, P_inv, synthetic.load_plane_database('100').astype(np.float32), P_raw)


def test_run_network_saves_device_composites(tmp_path, monkeypatch):
    """ bin/run_network.py --device-pose --save-images: one PNG per image, equal to the host renderer applied to the rows the run wrote its files from """
    from PIL import Image
    from keras_retinanet_3D.bin import run_network
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    (tmp_path / 'img').mkdir(); (tmp_path / 'calib').mkdir(); (tmp_path / 'dev').mkdir(); (tmp_path / 'host').mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    frames = {}
    for k, (h, w) in enumerate([(375, 1242), (370, 1224), (375, 1242)]):
        frames['%06d.png' % k] = noise_frames([(h, w)], seed=k)[0]
        Image.fromarray(frames['%06d.png' % k][:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    seen = {}
    original = run_network.write_results_from_rows

    def spy(args, output_dir, item, rows_b, count, picture=None):
        assert picture is not None
        seen[os.path.basename(item['image_fp'])] = (np.array(rows_b), int(count), run_network.raw_calibration(item))
        return original(args, output_dir, item, rows_b, count, picture)

    monkeypatch.setattr(run_network, 'write_results_from_rows', spy)
    common = ['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('1k')]
    run_network.main(common + [str(tmp_path / 'dev'), '--batch-size', '3', '--device-pose', '--save-images', '--image-score-threshold', '0.05'])
    assert sorted(seen) == sorted(frames)
    drawn = 0
    for name, frame in frames.items():
        path = tmp_path / 'dev' / 'synthetic:1234' / 'images' / 'composite' / name
        assert path.is_file()
        got = np.asarray(Image.open(str(path)).convert('RGB'))[:, :, ::-1]
        rows_b, count, P_raw = seen[name]
        assert np.array_equal(got, vis.composite_from_rows(frame, rows_b, count, P_raw, 0.05))
        drawn += int(not np.array_equal(got, np.vstack((frame, frame))))
    assert drawn > 0
    # the host path writes its pictures too
    run_network.main(common + [str(tmp_path / 'host'), '--batch-size', '3', '--save-images', '--image-score-threshold', '0.05'])
    for name, frame in frames.items():
        path = tmp_path / 'host' / 'synthetic:1234' / 'images' / 'composite' / name
        assert path.is_file() and np.asarray(Image.open(str(path))).shape == (2 * frame.shape[0], frame.shape[1], 3)
