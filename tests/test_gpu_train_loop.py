"""GPU: train_net / train_net_alter end to end on a few small in-memory images -- real network, data layers, train
steps, validation pass, snapshots, log files and the device-drawn pictures -- and resume.

Resume is checked on what is deterministic by construction: the restored parameters and optimiser state are the saved
bits, and every mini-batch the resumed run feeds its steps is bit for bit the one the uninterrupted run fed at the same
iteration (the permutations, cursors and NumPy stream are restored; the image op is deterministic).  The same state and
the same inputs are the same computation; no tolerance on trained weights is needed."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSES = ['__background__', 'benign', 'malignant']


def entry(seed, h, w, diag, flipped=False):
    rs = np.random.RandomState(seed)
    plane = np.clip(rs.rayleigh(40.0, size=(h, w)), 0, 255).astype(np.uint8)
    x, y = int(rs.randint(5, w // 2)), int(rs.randint(5, h // 2))
    boxes = np.asarray([[x, y, x + int(rs.randint(30, w // 2 - 5)), y + int(rs.randint(30, h // 2 - 5))]], np.uint16)
    return dict(plane=plane, flipped=flipped, boxes=boxes, gt_classes=np.asarray([1 + diag], np.int32), birads_diag=diag, height=h,
                width=w, image='img_%03d.tif' % seed)


class Imdb(object):
    num_classes, classes = 3, CLASSES

    def __init__(self, roidb):
        self.roidb = roidb

    def image_path_at(self, i):
        return os.path.join('/data/TIFFImages', self.roidb[i]['image'])


@pytest.fixture
def setup(monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from wssdl_bus_amd.fast_rcnn.config import cfg
    for k, v in dict(SCALES=(160,), MAX_SIZE=300, IMS_PER_BATCH=1, WS_IMS_PER_BATCH=1, DISPLAY=1, SNAPSHOT_ITERS=2, TEST_ITERS=2,
                     SNAPSHOT_INFIX='', WS_TRAIN_INTERVAL=1).items():
        monkeypatch.setattr(cfg.TRAIN, k, v)
    monkeypatch.setattr(cfg.TEST, "SCALES", (160,))
    monkeypatch.setattr(cfg.TEST, "MAX_SIZE", 300)
    state = np.random.get_state()
    yield cfg
    np.random.set_state(state)


def datasets():
    roidb_s = [entry(10 + i, 100 + 7 * i, 150 - 9 * i, i % 2, i == 2) for i in range(3)]
    roidb_ws = [entry(20 + i, 120 - 5 * i, 140 + 3 * i, (i + 1) % 2) for i in range(3)]
    roidb_t = [entry(30 + i, 96 + 11 * i, 131 + 6 * i, i % 2) for i in range(3)]
    return roidb_s, roidb_ws, roidb_t


def make_net(torch, name):
    from wssdl_bus_amd.networks.factory_bus import get_network
    torch.manual_seed(7)
    net = get_network(name, 18).cuda().to(memory_format=torch.channels_last)
    net.train()
    return net


def run(torch, train_fn, name, out, max_iters, **kw):
    """-> (history, the [data blob per train-step forward] the run fed, the network)"""
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper
    roidb_s, roidb_ws, roidb_t = datasets()
    fed, originals = [], {}
    for method in ('train_step_joint', 'supervised_backward', 'weak_backward'):
        orig = originals[method] = getattr(SolverWrapper, method)

        def wrapped(self, blobs, _orig=orig):
            fed.append(blobs['data'].clone())
            return _orig(self, blobs)
        setattr(SolverWrapper, method, wrapped)
    try:
        np.random.seed(3)
        net = make_net(torch, name)
        hist = train_fn(net, Imdb(roidb_s), roidb_s, Imdb(roidb_ws), roidb_ws, Imdb(roidb_t), roidb_t, str(out), max_iters=max_iters,
                        val_ims_per_batch=2, **kw)
    finally:
        for method, orig in originals.items():
            setattr(SolverWrapper, method, orig)
    return hist, fed, net


def test_joint_loop_end_to_end_with_pictures_and_resume(setup, monkeypatch, tmp_path):
    import torch
    from wssdl_bus_amd.fast_rcnn import snapshot, vis
    from wssdl_bus_amd.fast_rcnn.train_bus import train_net
    out = tmp_path / 'run'
    hist, fed, net = run(torch, train_net, 'Resnet_train', out, 4, vis=True)
    # files
    names = sorted(os.listdir(str(out)))
    assert names == ['Resnet_fast_rcnn_iter_2.pt', 'Resnet_fast_rcnn_iter_4.pt', 'log.txt', 'summary.jsonl', 'test']
    assert sorted(os.listdir(str(out / 'test'))) == ['img_030.png', 'img_031.png', 'img_032.png']
    log = open(str(out / 'log.txt')).read().splitlines()
    assert len(log) == 20 and log[0] == 'iter: 2 / 4' and log[10] == 'iter: 4 / 4' and log[9] == 'lr: 0.0005'
    assert log[8] == 'mil_loss_cls: 0.0'                                    # the joint loop's test MIL slot
    recs = [json.loads(l) for l in open(str(out / 'summary.jsonl'))]
    assert [r['iter'] for r in recs] == [2, 4] and all(np.isfinite(r['training_loss_total']) and r['training_loss_total'] > 0 for r in recs)
    assert all(np.isfinite(r['test_loss_total']) for r in recs)
    # the history keeps validate's whole result; the pictures are the painter's pictures of its detections
    assert [v['iter'] for v in hist['validations']] == [2, 4] and len(fed) == 4
    result = hist['validations'][-1]['result']
    assert result['n_images'] == 3 and result['per_image'].shape == (3, 6)
    _, _, roidb_t = datasets()
    dets, counts = (t.cpu().numpy() for t in result['detections'].gathered(3))
    colours, glyphs = vis.colour_table(CLASSES), vis.glyph_table()
    for i, e in enumerate(roidb_t):
        pic = ref.decode_png(open(str(out / 'test' / ('img_%03d.png' % (30 + i))), 'rb').read())
        want = ref.paint_image(e['plane'], e['boxes'], e['gt_classes'], dets[i], counts[i], colours, glyphs, CLASSES)
        assert pic.shape == e['plane'].shape + (3,) and np.array_equal(pic, want)
        assert (pic == (255, 0, 0)).all(axis=2).any() or (pic == (0, 0, 255)).all(axis=2).any()      # the ground truth at least

    # resume from the snapshot of iteration 2 into a fresh network
    path = str(out / 'Resnet_fast_rcnn_iter_2.pt')
    saved = snapshot.load_file(path)
    assert saved['iteration'] == 1 and saved['global_step'] == 2 and saved['loop']['pending_validation'] is True
    hist2, fed2, net2 = run(torch, train_net, 'Resnet_train', tmp_path / 'resumed', 4, vis=False, resume=path)
    assert len(fed2) == 2 and all(torch.equal(a, b) for a, b in zip(fed2, fed[2:]))
    assert [v['iter'] for v in hist2['validations']] == [2, 4]              # the pending pass first, then iteration 4's
    assert [os.path.basename(p) for p in hist2['snapshots']] == ['Resnet_fast_rcnn_iter_4.pt']
    end = snapshot.load_file(hist2['snapshots'][0])
    full = snapshot.load_file(str(out / 'Resnet_fast_rcnn_iter_4.pt'))
    assert end['global_step'] == full['global_step'] == 4
    for k in ('train',):
        for name in ('perm_s', 'perm_ws'):
            assert np.array_equal(end['data_layers'][k][name], full['data_layers'][k][name])
        assert end['data_layers'][k]['cur_s'] == full['data_layers'][k]['cur_s']
    assert np.array_equal(end['rng']['numpy'][1], full['rng']['numpy'][1]) and end['rng']['numpy'][2] == full['rng']['numpy'][2]
    assert not os.path.exists(str(tmp_path / 'resumed' / 'test'))


def test_restore_puts_back_the_saved_bits(setup, monkeypatch, tmp_path):
    import torch
    from wssdl_bus_amd.fast_rcnn import snapshot
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper, train_net_alter
    monkeypatch.setattr(setup.TRAIN, "SNAPSHOT_ITERS", 1)
    hist, fed, net = run(torch, train_net_alter, 'Resnet_train_alter', tmp_path, 2, vis=False)
    assert len(fed) == 4                                                    # a supervised and a weak forward per iteration
    assert [os.path.basename(p) for p in hist['snapshots']] == ['Resnet_fast_rcnn_iter_1.pt', 'Resnet_fast_rcnn_iter_2.pt']
    v = hist['validations'][0]
    assert v['iter'] == 2 and v['result']['mil_cross_entropy'] >= 0 and len(v['result']['corloc_list']) == 3
    log = open(str(tmp_path / 'log.txt')).read().splitlines()
    assert log[8] == 'mil_loss_cls: ' + str(float(v['result']['mil_cross_entropy']))
    # restore the last snapshot into fresh objects: parameters, buffers and both optimisers' moments are the final bits
    fresh = make_net(torch, 'Resnet_train_alter')
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    solver = SolverWrapper(fresh, 5e-4, None, 'adam', 'const', 2)
    it, loop = snapshot.restore(hist['snapshots'][-1], solver, {}, rank_local=True)
    assert it == 2 and solver.global_step == 2 and solver.optimizer_ws is not None
    a, b = net.state_dict(), fresh.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    saved = snapshot.load_file(hist['snapshots'][-1])
    assert solver.optimizer.state_dict()['step'] == saved['optimizer']['step'] == 2
    assert solver.optimizer_ws.state_dict()['step'] == saved['optimizer_ws']['step'] == 2
    assert torch.equal(torch.cuda.get_rng_state(), saved['rng']['torch_device'])
    with pytest.raises(ValueError, match="resume"):
        snapshot.restore(hist['snapshots'][-1], SolverWrapper(fresh, 5e-4, None, 'sgd', 'const', 2), {})
