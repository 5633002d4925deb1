"""CPU: the training loops of fast_rcnn/train_loop.py and the snapshots of fast_rcnn/snapshot.py with a stub solver and
stub data layers that record their calls: which iterations display, snapshot and validate, the alternating windows,
the stand-in values, log.txt character for character, the summary keys, the snapshot names, check_flags before every
write, resume; the running means against a sequential f64 host sum; the data layers' state_dict round trip."""
import json
import math
import os

import numpy as np
import pytest
import torch

from wssdl_bus_amd.fast_rcnn import snapshot, train_loop
from wssdl_bus_amd.fast_rcnn.config import cfg


class Stubnet_bus(object):
    alter = True

    def __init__(self):
        self.w = torch.zeros(3)

    def state_dict(self):
        return {'w': self.w.clone()}

    def load_state_dict(self, sd, strict=True):
        self.w = sd['w'].clone()


class StubOptimizer(object):
    def __init__(self):
        self.steps = 0

    def state_dict(self):
        return {'steps': self.steps}

    def load_state_dict(self, sd):
        self.steps = int(sd['steps'])


class StubLayer(object):
    def __init__(self, name, log):
        self.name, self.log, self.n = name, log, 0

    def forward(self):
        self.n += 1
        self.log.append(('forward', self.name))
        return {'n': self.n}

    def state_dict(self):
        return {'n': self.n}

    def load_state_dict(self, sd):
        self.n = int(sd['n'])


def sup_values(k):
    """The four supervised terms of the k-th supervised call (k from 1), as f32."""
    return [np.float32(0.1 * k + 0.013), np.float32(0.2 + 0.01 * k), np.float32(1.0 / (k + 2)), np.float32(0.05 * k * k)]


def mil_value(k):
    return np.float32(0.7 + 0.003 * k)


class StubSolver(object):
    def __init__(self, opt='adam', lr=5e-4, lr_scheduling='const', max_iters=7, flags_raise_at=None):
        self.net = Stubnet_bus()
        self.opt, self.lr, self.lr_scheduling, self.max_iters = opt, lr, lr_scheduling, max_iters
        self.optimizer, self.optimizer_ws = StubOptimizer(), None
        self.global_step, self.rop, self.dist = 0, None, None
        self.log, self.n_sup, self.n_ws, self.n_flags = [], 0, 0, 0
        self.flags_raise_at = flags_raise_at

    def current_lr(self):
        return self.lr

    def _make_optimizer(self):
        return StubOptimizer()

    def supervised_backward(self, blobs):
        self.n_sup += 1
        self.log.append(('sup', blobs['n']))
        v = sup_values(self.n_sup)
        return dict(zip(train_loop.SUP_TERMS, [torch.tensor(x) for x in v]))

    def weak_backward(self, blobs):
        self.n_ws += 1
        self.log.append(('ws', blobs['n']))
        return torch.tensor(mil_value(self.n_ws))

    def train_step_joint(self, blobs):
        self.n_sup += 1
        self.n_ws += 1
        self.log.append(('joint', blobs['n']))
        out = dict(zip(train_loop.SUP_TERMS, [torch.tensor(x) for x in sup_values(self.n_sup)]))
        out['mil_cross_entropy'] = torch.tensor(mil_value(self.n_ws))
        self._apply()
        return out

    def _apply(self, optimizer=None, count_step=True):
        optimizer = optimizer or self.optimizer
        optimizer.steps += 1
        self.net.w = self.net.w + 1
        self.log.append(('apply', 'ws' if optimizer is self.optimizer_ws else 's', bool(count_step)))
        if count_step:
            self.global_step += 1

    def check_flags(self):
        self.n_flags += 1
        self.log.append(('check_flags',))
        if self.flags_raise_at is not None and self.n_flags >= self.flags_raise_at:
            raise RuntimeError("device flag raised")

    def on_val_end(self, v):
        self.log.append(('on_val_end', v))


class Imdb(object):
    num_classes = 3
    classes = ['__background__', 'benign', 'malignant']


TEST_RESULT = dict(total=1.5, rpn_cross_entropy=0.25, rpn_loss_box=0.125, cross_entropy=0.75, loss_box=0.375, mil_cross_entropy=0.0625,
                   corloc_list=[0.5, 0.25, 0.375], n_images=2)


def make_test_pass(solver):
    def test_pass(s, imdb_test, roidb_test, net_name, val_ims_per_batch, thresh, max_per_image, vis, output_dir):
        solver.log.append(('validate', thresh, max_per_image, val_ims_per_batch))
        return dict(TEST_RESULT)
    return test_pass


@pytest.fixture
def schedule():
    old = {k: cfg.TRAIN[k] for k in ('DISPLAY', 'SNAPSHOT_ITERS', 'TEST_ITERS', 'WS_TRAIN_INTERVAL', 'SNAPSHOT_INFIX')}
    cfg.TRAIN.DISPLAY, cfg.TRAIN.SNAPSHOT_ITERS, cfg.TRAIN.TEST_ITERS = 1, 2, 3
    yield
    for k, v in old.items():
        cfg.TRAIN[k] = v


def run_alter(tmp_path, solver=None, max_iters=7, windows=(0, 80000, 0, 80000), resume=None, layers=None):
    solver = solver or StubSolver(max_iters=max_iters)
    layers = layers or dict(train_s=StubLayer('s', solver.log), train_ws=StubLayer('ws', solver.log))
    hist = train_loop.train_model_alter(solver, Imdb(), [], Imdb(), [], Imdb(), [], str(tmp_path), max_iters, *windows, resume=resume,
                                        data_layers=layers, test_pass=make_test_pass(solver))
    return solver, hist, layers


def run_joint(tmp_path, solver=None, max_iters=7, resume=None):
    solver = solver or StubSolver(max_iters=max_iters)
    layers = dict(train=StubLayer('joint', solver.log))
    hist = train_loop.train_model(solver, Imdb(), [], Imdb(), [], Imdb(), [], str(tmp_path), max_iters, 3, 4, 5, 6, resume=resume,
                                  data_layers=layers, test_pass=make_test_pass(solver))
    return solver, hist, layers


def test_config_keys_are_the_references():
    assert (cfg.TRAIN.DISPLAY, cfg.TRAIN.SNAPSHOT_ITERS, cfg.TRAIN.TEST_ITERS, cfg.TRAIN.SNAPSHOT_INFIX, cfg.TRAIN.WS_TRAIN_INTERVAL) == \
        (10, 10, 10, '', 1)


def test_which_iterations_display_snapshot_and_validate(tmp_path, schedule, capsys):
    solver, hist, _ = run_alter(tmp_path)
    out = capsys.readouterr().out
    assert [l for l in out.splitlines() if l.startswith('iter: ')].count('iter: 7 / 7') == 1
    assert out.count('speed: ') == 7                                        # DISPLAY = 1
    assert out.count('training loss') == 2 and out.count('Wrote snapshot to: ') == 4
    names = [os.path.basename(p) for p in hist['snapshots']]
    assert names == ['Stubne_fast_rcnn_iter_%d.pt' % i for i in (2, 4, 6, 7)]      # every 2nd, and the final one
    assert [v['iter'] for v in hist['validations']] == [3, 6]
    assert sorted(os.listdir(str(tmp_path))) == sorted(names + ['log.txt', 'summary.jsonl'])
    # check_flags before every write, and once more at the end of training
    assert solver.log.count(('check_flags',)) == 5 and solver.log[-1] == ('check_flags',)
    # at iteration 6 (0-based 5) the snapshot precedes the validation pass, as in the reference
    i_val = [i for i, e in enumerate(solver.log) if e[0] == 'validate']
    assert solver.log[i_val[1] - 1] == ('check_flags',)
    assert solver.log[i_val[0]] == ('validate', 0.05, 300, 1)
    # every iteration: a supervised step that does not count, then a weak step that does
    steps = [e for e in solver.log if e[0] == 'apply']
    assert steps == [('apply', 's', False), ('apply', 'ws', True)] * 7 and solver.global_step == 7
    assert hist['validations'][0]['result']['corloc_list'] == [0.5, 0.25, 0.375] and hist['validations'][0]['lr'] == 5e-4


def test_sgd_counts_both_halves(tmp_path, schedule):
    solver, _, _ = run_alter(tmp_path, StubSolver(opt='sgd', max_iters=3), max_iters=3)
    assert [e for e in solver.log if e[0] == 'apply'] == [('apply', 's', True), ('apply', 'ws', True)] * 3
    assert solver.global_step == 6


def test_final_snapshot_only_when_the_last_iteration_took_none(tmp_path, schedule):
    _, hist, _ = run_alter(tmp_path, max_iters=4)
    assert [os.path.basename(p) for p in hist['snapshots']] == ['Stubne_fast_rcnn_iter_2.pt', 'Stubne_fast_rcnn_iter_4.pt']


def test_snapshot_name_with_infix(tmp_path, schedule):
    cfg.TRAIN.SNAPSHOT_INFIX = 'run2'
    _, hist, _ = run_alter(tmp_path, max_iters=2)
    assert [os.path.basename(p) for p in hist['snapshots']] == ['Stubne_fast_rcnn_run2_iter_2.pt']
    assert snapshot.snapshot_path('out', 'Resnet_train_bus', 9) == os.path.join('out', 'Resnet_fast_rcnn_run2_iter_10.pt')
    cfg.TRAIN.SNAPSHOT_INFIX = ''
    assert snapshot.snapshot_path('out', 'VGGnet_train_bus', 0) == os.path.join('out', 'VGGnet_fast_rcnn_iter_1.pt')


def expected_alter_means(max_iters, windows, interval, test_iters, num_classes=3):
    """The reference's arithmetic (:331-405, :529, :585-586) in plain Python floats, sequentially."""
    s0, s1, w0, w1 = windows
    training, old = [0.0] * 6, [0.0] * 6
    n_sup = n_ws = 0
    means, calls = [], []
    for it in range(max_iters):
        if s0 <= it <= s1:
            n_sup += 1
            a, b, c, d = (float(x) for x in sup_values(n_sup))
            calls.append(('sup', it))
        else:
            a, b, c, d = old[1], old[2], old[3], old[4]
        if w0 <= it <= w1 and (it + 1) % interval == 0:
            n_ws += 1
            m = float(mil_value(n_ws))
            calls.append(('ws', it))
        else:
            m = old[5] if old[5] != 0 else -math.log(1. / num_classes)
        for k, v in enumerate([a + b + c + d, a, b, c, d, m]):
            training[k] += v
        if (it + 1) % test_iters == 0:
            training = [v / test_iters for v in training]
            means.append(training)
            old, training = training, [0.0] * 6
    return means, calls


@pytest.mark.parametrize("windows, interval", [((0, 80000, 0, 80000), 1), ((0, 80000, 0, 80000), 2), ((2, 4, 1, 5), 2), ((7, 9, 0, 2), 1),
                                               ((0, 3, 9, 9), 1)])
def test_alternating_windows_standins_and_means(tmp_path, schedule, windows, interval):
    cfg.TRAIN.WS_TRAIN_INTERVAL = interval
    max_iters = 9
    solver, hist, layers = run_alter(tmp_path, StubSolver(max_iters=max_iters), max_iters=max_iters, windows=windows)
    want, calls = expected_alter_means(max_iters, windows, interval, 3)
    # a skipped half takes no batch from its data layer and no optimiser step
    assert layers['train_s'].n == solver.n_sup == sum(1 for c in calls if c[0] == 'sup')
    assert layers['train_ws'].n == solver.n_ws == sum(1 for c in calls if c[0] == 'ws')
    assert sum(1 for e in solver.log if e[0] == 'apply') == len(calls)
    got = [v['training_loss'] for v in hist['validations']]
    assert len(got) == len(want) == 3
    # reordering n f64 additions of same-sign terms moves the sum by at most 2 (n - 1) 2^-53 relative.  A component's
    # mean: its 3 terms and the join of the device and host (stand-in) parts, n = 4; the total's: 4 terms each, n = 13
    for g, w in zip(got, want):
        for k, (a, b) in enumerate(zip(g, w)):
            n = 13 if k == 0 else 4
            assert abs(a - b) <= 2 * (n - 1) * 2.0 ** -53 * abs(b), (k, g, w)
    if windows == (0, 3, 9, 9):                                            # the MIL term never ran: -log(1/3) throughout
        assert all(abs(g[5] - math.log(3.0)) < 1e-15 for g in got)


def test_joint_loop_ignores_the_windows_and_writes_zero_mil(tmp_path, schedule):
    solver, hist, layers = run_joint(tmp_path)
    assert layers['train'].n == 7 and solver.n_sup == 7                     # windows (3, 4, 5, 6) would have cut it short
    assert [e for e in solver.log if e[0] == 'apply'] == [('apply', 's', True)] * 7
    lines = open(os.path.join(str(tmp_path), 'log.txt')).read().splitlines()
    assert lines[8] == 'mil_loss_cls: 0.0'                                    # the joint loop's test MIL slot (:885)
    recs = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'summary.jsonl'))]
    assert recs[0]['test_loss_mil_loss_cls'] == 0 and recs[0]['training_loss_mil_loss_cls'] > 0


def test_log_txt_character_for_character_and_summary_keys(tmp_path, schedule):
    _, hist, _ = run_alter(tmp_path)
    means, _ = expected_alter_means(7, (0, 80000, 0, 80000), 1, 3)
    want = ''
    for it, tr in zip((3, 6), hist and [v['training_loss'] for v in hist['validations']]):
        want += 'iter: %d / 7\n' % it
        want += 'training loss\n'
        want += 'total_loss: ' + str(tr[0]) + '\n'
        want += 'rpn_loss_cls: ' + str(tr[1]) + '\trpn_loss_box: ' + str(tr[2]) + '\tloss_cls: ' + str(tr[3]) + '\tloss_box: ' + str(tr[4]) + '\n'
        want += 'mil_loss_cls: ' + str(tr[5]) + '\n'
        want += 'test loss\n'
        want += 'total_loss: 1.5\n'
        want += 'rpn_loss_cls: 0.25\trpn_loss_box: 0.125\tloss_cls: 0.75\tloss_box: 0.375\n'
        want += 'mil_loss_cls: 0.0625\n'
        want += 'lr: 0.0005\n'
    assert open(os.path.join(str(tmp_path), 'log.txt')).read() == want
    for tr, m in zip([v['training_loss'] for v in hist['validations']], means):
        assert np.allclose(tr, m, rtol=1e-14, atol=0)
    recs = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'summary.jsonl'))]
    assert [r['iter'] for r in recs] == [3, 6]
    assert set(recs[0]) == {'iter', 'lr', 'corloc for benign', 'corloc for malignant', 'corloc'} | set(train_loop.TRAIN_TAGS) | \
        set(train_loop.TEST_TAGS)
    assert recs[1]['test_loss_total'] == 1.5 and recs[1]['corloc'] == 0.375 and recs[1]['lr'] == 5e-4


def test_raised_flag_leaves_no_file(tmp_path, schedule):
    solver = StubSolver(max_iters=4, flags_raise_at=2)
    with pytest.raises(RuntimeError, match="device flag raised"):
        run_alter(tmp_path, solver, max_iters=4)
    left = sorted(os.listdir(str(tmp_path)))
    assert left == ['Stubne_fast_rcnn_iter_2.pt', 'log.txt', 'summary.jsonl']      # the second snapshot: nothing, no temporary


def test_resume_continues_where_the_snapshot_was_taken(tmp_path, schedule):
    full, hist_full, _ = run_alter(tmp_path / 'full')
    first, hist_a, _ = run_alter(tmp_path / 'two', max_iters=7)
    path = [p for p in hist_a['snapshots'] if p.endswith('_iter_4.pt')][0]
    solver = StubSolver(max_iters=7)
    layers = dict(train_s=StubLayer('s', solver.log), train_ws=StubLayer('ws', solver.log))
    solver.n_sup = solver.n_ws = 4                                          # the stub's own value counters are not solver state
    _, hist_b, layers = run_alter(tmp_path / 'two', solver, resume=path, layers=layers)
    assert layers['train_s'].n == 7 and solver.global_step == 7 and solver.optimizer.steps == 7 and solver.optimizer_ws.steps == 7
    assert torch.equal(solver.net.w, full.net.w)
    assert [v['iter'] for v in hist_b['validations']] == [6]
    assert hist_b['validations'][0]['training_loss'] == hist_full['validations'][1]['training_loss']
    assert [os.path.basename(p) for p in hist_b['snapshots']] == ['Stubne_fast_rcnn_iter_6.pt', 'Stubne_fast_rcnn_iter_7.pt']
    # a snapshot taken at a validating iteration precedes the pass: the resumed run validates first
    solver = StubSolver(max_iters=7)
    solver.n_sup = solver.n_ws = 6
    path6 = [p for p in hist_a['snapshots'] if p.endswith('_iter_6.pt')][0]
    _, hist_c, _ = run_alter(tmp_path / 'two', solver, resume=path6)
    assert [v['iter'] for v in hist_c['validations']] == [6]
    assert hist_c['validations'][0]['training_loss'] == hist_full['validations'][1]['training_loss']
    assert solver.log[0] == ('validate', 0.05, 300, 1)


def test_resume_with_other_settings_raises(tmp_path, schedule):
    _, hist, _ = run_alter(tmp_path, max_iters=2)
    for kw in (dict(opt='sgd'), dict(lr=1e-3), dict(lr_scheduling='pc'), dict(max_iters=9)):
        args = dict(max_iters=2)
        args.update(kw)
        with pytest.raises(ValueError, match="resume"):
            run_alter(tmp_path, StubSolver(**args), max_iters=2, resume=hist['snapshots'][0])


def test_snapshot_holds_rng_and_sampler_counters(tmp_path, schedule):
    from wssdl_bus_amd.rpn_msr import anchor_target_layer_tf_bus as atl, proposal_target_layer_tf_bus as ptl
    old = (atl.get_device_calls(), ptl.get_device_calls(), cfg.DEVICE_RNG_SEED, np.random.get_state(), torch.get_rng_state())
    try:
        atl.set_device_calls(17), ptl.set_device_calls(23)
        cfg.DEVICE_RNG_SEED = 41
        np.random.seed(5), torch.manual_seed(6)
        solver = StubSolver()
        path = snapshot.save_snapshot(solver, str(tmp_path), 'Stubnet_bus', 0, dict(running=train_loop.RunningLosses().state_dict()), {})
        want = (np.random.rand(3), torch.rand(3))
        atl.set_device_calls(0), ptl.set_device_calls(0)
        cfg.DEVICE_RNG_SEED = 3
        it, loop = snapshot.restore(path, StubSolver(), {})
        assert it == 1 and (atl.get_device_calls(), ptl.get_device_calls(), cfg.DEVICE_RNG_SEED) == (17, 23, 41)
        assert np.array_equal(np.random.rand(3), want[0]) and torch.equal(torch.rand(3), want[1])
        state = snapshot.load_file(path)
        assert {'model', 'optimizer', 'optimizer_ws', 'global_step', 'opt', 'lr', 'lr_scheduling', 'max_iters', 'rop', 'loop',
                'data_layers', 'rng', 'iteration'} <= set(state)
    finally:
        atl.set_device_calls(old[0]), ptl.set_device_calls(old[1])
        cfg.DEVICE_RNG_SEED = old[2]
        np.random.set_state(old[3]), torch.set_rng_state(old[4])


def test_pretrained_model_is_loaded_non_strictly(tmp_path, capsys):
    net = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Linear(2, 1))
    sd = {k: v + 1 for k, v in net.state_dict().items() if not k.startswith('1.')}
    path = str(tmp_path / 'w.pt')
    torch.save(sd, path)
    missing = snapshot.load_pretrained(net, path)
    assert sorted(missing) == ['1.bias', '1.weight'] and torch.equal(net.state_dict()['0.weight'], sd['0.weight'])
    assert 'ignore missing: 1.weight' in capsys.readouterr().out


def test_real_solver_snapshot_round_trip(tmp_path):
    """SolverWrapper on a small CPU module: parameters, both optimisers, the step and the plateau state come back."""
    from wssdl_bus_amd.fast_rcnn.train_bus import SolverWrapper

    class Tinynet_bus(torch.nn.Linear):
        pass

    def make():
        torch.manual_seed(0)
        s = SolverWrapper(Tinynet_bus(3, 2), 1e-3, None, None, 'rop', 10)
        s.check_flags = lambda: None                                        # (the device flags need the library's GPU side)
        return s
    a = make()
    a.optimizer_ws = a._make_optimizer()
    for opt in (a.optimizer, a.optimizer_ws, a.optimizer):
        a.net(torch.ones(1, 3)).sum().backward()
        opt.step()
        a.optimizer.zero_grad()
    a.global_step = 5
    for v in (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0):
        a.on_val_end(v)
    path = snapshot.save_snapshot(a, str(tmp_path), 'Tinynet_bus', 4, dict(x=1), {})
    assert os.path.basename(path) == 'Tinyne_fast_rcnn_iter_5.pt'
    b = make()
    it, loop = snapshot.restore(path, b, {})
    assert it == 5 and loop == dict(x=1) and b.global_step == 5
    assert all(torch.equal(p, q) for p, q in zip(a.net.state_dict().values(), b.net.state_dict().values()))
    assert b.current_lr() == a.current_lr() < 1e-3 and b.rop.wait == a.rop.wait and b.rop.best == a.rop.best
    sa, sb = a.optimizer.state_dict()['state'], b.optimizer.state_dict()['state']
    assert all(torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']) for k in sa) and b.optimizer_ws is not None
    assert float(b.optimizer_ws.state_dict()['state'][0]['step']) == 1.0 and float(sb[0]['step']) == 2.0


def _roidb(n):
    return [dict(idx=i) for i in range(n)]


def test_data_layer_state_round_trip():
    from wssdl_bus_amd.roi_data_layer.layer_bus import RoIDataLayer
    from wssdl_bus_amd.roi_data_layer.layer_bus_joint import RoIDataLayerJoint
    old = (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH, np.random.get_state())
    try:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = 2, 3
        np.random.seed(9)
        a = RoIDataLayer(_roidb(7), 'Resnet_train_bus', 3, True, False)
        for _ in range(2):
            a._get_next_minibatch_inds()
        state, rng = a.state_dict(), np.random.get_state()
        want = [a._get_next_minibatch_inds().tolist() for _ in range(5)]     # crosses a re-permutation (7 entries, 2 per batch)
        b = RoIDataLayer(_roidb(7), 'Resnet_train_bus', 3, True, False)
        b.load_state_dict(state)
        np.random.set_state(rng)
        assert [b._get_next_minibatch_inds().tolist() for _ in range(5)] == want
        assert len({tuple(w) for w in want}) > 1
        with pytest.raises(ValueError):
            RoIDataLayer(_roidb(6), 'Resnet_train_bus', 3, True, False).load_state_dict(state)

        j = RoIDataLayerJoint(_roidb(5), _roidb(7), 'Resnet_train_bus', 3, True)
        j._get_next_minibatch_inds()
        state, rng = j.state_dict(), np.random.get_state()
        want = [[x.tolist() for x in j._get_next_minibatch_inds()] for _ in range(5)]
        k = RoIDataLayerJoint(_roidb(5), _roidb(7), 'Resnet_train_bus', 3, True)
        k.load_state_dict(state)
        np.random.set_state(rng)
        assert [[x.tolist() for x in k._get_next_minibatch_inds()] for _ in range(5)] == want
        # the state is a copy: drawing on does not change what was saved
        assert state['cur_s'] == 2 and state['cur_ws'] == 3
    finally:
        cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.WS_IMS_PER_BATCH = old[0], old[1]
        np.random.set_state(old[2])


def test_cfg_from_list_sets_the_new_keys():
    from wssdl_bus_amd.fast_rcnn.config import cfg_from_list
    old = cfg.TRAIN.TEST_ITERS, cfg.TRAIN.SNAPSHOT_INFIX
    try:
        cfg_from_list(['TRAIN.TEST_ITERS', '25', 'TRAIN.SNAPSHOT_INFIX', 'abc'])
        assert cfg.TRAIN.TEST_ITERS == 25 and cfg.TRAIN.SNAPSHOT_INFIX == 'abc'
    finally:
        cfg.TRAIN.TEST_ITERS, cfg.TRAIN.SNAPSHOT_INFIX = old
