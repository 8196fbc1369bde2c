"""CPU tests of the training harness's control flow (chem_model.ChemModel.run_epoch / train / save_progress / restore_progress):
patience and best epoch, the log, the epoch arithmetic, resume, the configuration check of a checkpoint, --quiet and the
single writer under data parallelism.  The model is a real SparseGGNNChemModel on the CPU; its batch iterator and its two
per-batch entry points are replaced by scripted ones, so no kernel runs."""
import json
import os
import pickle
import re
import threading
import types

import numpy as np
import pytest
import torch

CHEMICAL_ACCURACY = {0: 0.066513725, 3: 0.033730778}
TRAIN_SIZES, VALID_SIZES = (4, 7, 2), (3, 5)


class _Script:
    """Scripted batches: make_minibatch_iterator yields {'num_graphs': n}; forward_batch / train_batch fill
    ops['accuracy_task%i'] and return a scalar loss.  `mae(is_training, epoch, batch)` gives the per-task MAEs and
    `loss(is_training, epoch, batch)` the loss, epoch counting each kind of epoch from 0."""

    def __init__(self, model, mae, loss=None, train_sizes=TRAIN_SIZES, valid_sizes=VALID_SIZES):
        self.model, self.mae, self.loss = model, mae, loss or (lambda is_training, epoch, batch: 0.5 if is_training else 0.25)
        self.sizes = {True: tuple(train_sizes), False: tuple(valid_sizes)}
        self.calls = {True: 0, False: 0}
        self.epochs, self.on_main_thread, self.keep_probs, self.saves, self.prepared = [], [], [], [], []
        model.make_minibatch_iterator = self.batches
        model.forward_batch = lambda batch: self.step(False, batch)
        model.train_batch = lambda batch: self.step(True, batch)
        model.prepare_resident_data = lambda data, is_training: self.prepared.append(is_training)
        save = model.save_progress
        model.save_progress = lambda path, train_step, valid_step: (self.saves.append((self.epochs.count(True), train_step, valid_step)),
                                                                    save(path, train_step, valid_step))

    def batches(self, data, is_training):
        self.epochs.append(is_training)
        for n in self.sizes[is_training]:
            self.on_main_thread.append((is_training, threading.current_thread() is threading.main_thread()))
            yield {'num_graphs': n}

    def step(self, is_training, batch):
        epoch, i = divmod(self.calls[is_training], len(self.sizes[is_training]))
        self.calls[is_training] += 1
        assert batch['num_graphs'] == self.sizes[is_training][i]
        self.keep_probs.append((is_training, batch['out_layer_dropout_keep_prob']))
        for task_id, value in zip(self.model.params['task_ids'], self.mae(is_training, epoch, i)):
            self.model.ops['accuracy_task%i' % task_id] = torch.tensor(value, dtype=torch.float32)
        return torch.tensor(self.loss(is_training, epoch, i), dtype=torch.float32)


@pytest.fixture(scope="module")
def molecules(pkg):
    return pkg.synthetic_qm9(30, mean_nodes=8, seed=1)


def _model(pkg, molecules, log_dir=None, config=None, **args):
    config = dict({"threaded_batches": False}, **(config or {}))
    args = dict({"--device": "cpu", "train_data": molecules, "valid_data": molecules, "--config": config,
                 "--quiet": log_dir is None, "--log_dir": None if log_dir is None else str(log_dir)}, **args)
    return pkg.SparseGGNNChemModel(args)


def _valid_script(values):
    """MAE 1.0 on every training batch, values[epoch] on every batch of a validation epoch (single task)."""
    return lambda is_training, epoch, batch: [1.0] if is_training else [values[epoch]]


def test_patience_best_epoch_and_printed_text(pkg, molecules, tmp_path, capsys):
    m = _model(pkg, molecules, tmp_path, {"patience": 2, "num_epochs": 10})
    capsys.readouterr()
    s = _Script(m, _valid_script([3.0, 2.0, 2.5, 2.6, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]))
    log = m.train()
    assert len(log) == 4 and [e['epoch'] for e in log] == [1, 2, 3, 4]
    nt, nv = len(TRAIN_SIZES), len(VALID_SIZES)
    assert s.saves == [(1, nt, nv), (2, 2 * nt, 2 * nv)]
    assert (m.train_step_id, m.valid_step_id) == (4 * nt, 4 * nv)
    blob = pickle.load(open(m.best_model_file, "rb"))
    assert (blob["train_step"], blob["valid_step"]) == (2 * nt, 2 * nv)
    assert s.epochs == [True, False] * 4 and all(main for _, main in s.on_main_thread) and s.prepared == []
    # the program's output format, byte for byte (the speed is the one figure that varies)
    out = re.sub(r"instances/sec: [0-9.]+", "instances/sec: X", capsys.readouterr().out)
    ratio = lambda v: "%.5f" % (v / CHEMICAL_ACCURACY[0])
    want = ""
    for epoch, v in enumerate([3.0, 2.0, 2.5, 2.6], 1):
        want += "== Epoch %i\n" % epoch
        want += "".join("Running epoch %i (training), batch %i (has %i graphs). Loss so far: 0.5000\r" % (epoch, i, n)
                        for i, n in enumerate(TRAIN_SIZES))
        want += "\r\x1b[K Train: loss: 0.50000 | acc: 0:1.00000 | error_ratio: 0:%s | instances/sec: X\n" % ratio(1.0)
        want += "".join("Running epoch %i (validation), batch %i (has %i graphs). Loss so far: 0.2500\r" % (epoch, i, n)
                        for i, n in enumerate(VALID_SIZES))
        want += "\r\x1b[K Valid: loss: 0.25000 | acc: 0:%.5f | error_ratio: 0:%s | instances/sec: X\n" % (v, ratio(v))
        if epoch <= 2:
            want += "  (Best epoch so far, cum. val. acc decreased to %.5f from %s. Saving to '%s')\n" % (
                v, "inf" if epoch == 1 else "3.00000", m.best_model_file)
    want += "Stopping training after 2 epochs without improvement on validation accuracy.\n"
    assert out == want


def test_log_entries_and_files(pkg, molecules, tmp_path, capsys):
    m = _model(pkg, molecules, tmp_path, {"num_epochs": 3})
    start = capsys.readouterr().out
    assert start == "Run %s starting with following parameters:\n%s\n" % (m.run_id, json.dumps(m.params))
    _Script(m, _valid_script([3.0, 2.0, 2.5]))
    log = m.train()
    assert len(log) == 3
    for entry in log:
        assert set(entry) == {'epoch', 'time', 'train_results', 'valid_results'}
        assert type(entry['epoch']) is int and type(entry['time']) is float
        for result in (entry['train_results'], entry['valid_results']):
            loss, accs, errs, speed = result
            assert isinstance(loss, float) and isinstance(speed, float) and speed > 0
            assert type(accs) is list and type(errs) is list and len(accs) == len(errs) == 1
            assert all(type(x) is float for x in accs + errs)
    times = [e['time'] for e in log]
    assert times == sorted(times)
    assert [e['valid_results'][1] for e in log] == [[3.0], [2.0], [2.5]]
    assert m.log_file == os.path.join(str(tmp_path), "%s_log.json" % m.run_id)
    text = open(m.log_file).read()
    assert json.loads(text) == json.loads(json.dumps(log)) and text == json.dumps(log, indent=4)
    assert json.load(open(os.path.join(str(tmp_path), "%s_params.json" % m.run_id))) == m.params
    assert sorted(os.listdir(str(tmp_path))) == sorted("%s_%s" % (m.run_id, n) for n in ("log.json", "model_best.pickle", "params.json"))


@pytest.mark.parametrize("is_training", [True, False])
def test_epoch_arithmetic_weights_by_graph_count(pkg, molecules, is_training):
    m = _model(pkg, molecules, config={"task_ids": [0, 3], "out_layer_dropout_keep_prob": 0.5})
    sizes = (5, 11, 2)
    losses = [0.5, 0.25, 2.0]
    maes = [[1.0, 2.0], [3.0, 5.0], [0.5, 0.125]]                      # (all exact in float32)
    s = _Script(m, lambda t, e, i: maes[i], lambda t, e, i: losses[i], train_sizes=sizes, valid_sizes=sizes)
    loss, accs, errs, speed, steps = m.run_epoch("an epoch", m.train_data if is_training else m.valid_data, is_training, 5)
    n = np.array(sizes, dtype=np.float64)
    want_accs = (np.array(maes) * n[:, None]).sum(0) / n.sum()
    assert steps == 3 and speed > 0
    assert loss == pytest.approx(float((np.array(losses) * n).sum() / n.sum()), rel=1e-14)
    assert isinstance(accs, np.ndarray) and accs.shape == (2,) and np.allclose(accs, want_accs, rtol=1e-14, atol=0)
    assert np.allclose(errs, want_accs / np.array([CHEMICAL_ACCURACY[0], CHEMICAL_ACCURACY[3]]), rtol=1e-14, atol=0)
    assert s.keep_probs == [(is_training, 0.5 if is_training else 1.0)] * 3      # the readout's keep probability: training only
    assert s.epochs == [is_training]


def test_resume_scores_one_validation_epoch_first(pkg, molecules, tmp_path, capsys):
    path = str(tmp_path / "saved.pickle")
    _model(pkg, molecules).save_progress(path, 7, 3)
    logs = tmp_path / "logs"
    m = _model(pkg, molecules, logs, {"num_epochs": 2}, **{"--restore": path})
    assert (m.train_step_id, m.valid_step_id) == (7, 3)
    assert ("Restoring weights from file %s.\n" % path) in capsys.readouterr().out
    s = _Script(m, _valid_script([2.0, 2.5, 1.5]))
    log = m.train()
    nt, nv = len(TRAIN_SIZES), len(VALID_SIZES)
    assert s.epochs == [False, True, False, True, False] and len(log) == 2
    assert (m.train_step_id, m.valid_step_id) == (7 + 2 * nt, 3 + 3 * nv)
    assert s.saves == [(2, 7 + 2 * nt, 3 + 3 * nv)]                     # epoch 1 (2.5) does not beat the resumed 2.0
    out = capsys.readouterr().out
    assert "\r\x1b[KResumed operation, initial cum. val. acc: 2.00000\n== Epoch 1\n" in out
    assert "  (Best epoch so far, cum. val. acc decreased to 1.50000 from 2.00000. Saving to '%s')\n" % m.best_model_file in out
    # with patience 1 the resumed score counts as epoch 0's: one epoch without improvement ends the run
    _model(pkg, molecules, config={"patience": 1}).save_progress(path, 7, 3)
    m = _model(pkg, molecules, tmp_path / "logs2", {"num_epochs": 5, "patience": 1}, **{"--restore": path})
    s = _Script(m, _valid_script([2.0, 2.5, 1.5]))
    assert len(m.train()) == 1 and s.saves == []


def test_checkpoint_configuration_must_match(pkg, molecules, tmp_path):
    path = str(tmp_path / "saved.pickle")
    _model(pkg, molecules).save_progress(path, 7, 3)
    for key, value in (("learning_rate", 0.01), ("patience", 3), ("use_edge_bias", True)):
        with pytest.raises(AssertionError):
            _model(pkg, molecules, config={key: value}, **{"--restore": path})
    with pytest.raises(AssertionError):                                  # one key more than the checkpoint has
        _model(pkg, molecules, config={"multitask_readout": True}, **{"--restore": path})
    m = _model(pkg, molecules, config={"task_ids": [0, 3], "num_epochs": 5}, **{"--restore": path})
    assert (m.train_step_id, m.valid_step_id) == (7, 3)


def test_quiet_writes_no_file(pkg, molecules, tmp_path, capsys):
    m = _model(pkg, molecules, tmp_path, {"num_epochs": 2}, **{"--quiet": True})
    assert capsys.readouterr().out == ""
    s = _Script(m, _valid_script([3.0, 2.0]))
    assert len(m.train()) == 2
    assert os.listdir(str(tmp_path)) == [] and s.saves == []
    assert "Running" not in capsys.readouterr().out                      # no progress line either


def test_second_rank_writes_no_checkpoint(pkg, molecules, tmp_path):
    m = _model(pkg, molecules, tmp_path, {"num_epochs": 2}, dist=types.SimpleNamespace(active=False, rank=1, world_size=1))
    s = _Script(m, _valid_script([3.0, 2.0]))
    assert len(m.train()) == 2
    assert s.saves == [] and not os.path.exists(m.best_model_file)
    assert os.path.exists(m.log_file)


def test_threaded_batches_pack_training_epochs_on_a_thread(pkg, molecules):
    m = _model(pkg, molecules, config={"num_epochs": 2, "threaded_batches": True})
    s = _Script(m, _valid_script([3.0, 2.0]))
    log = m.train()
    assert len(log) == 2 and [e['valid_results'][1] for e in log] == [[3.0], [2.0]]
    assert s.prepared == [True, True]                                   # the resident data: before each training epoch only
    assert all(main != is_training for is_training, main in s.on_main_thread)
    assert (m.train_step_id, m.valid_step_id) == (2 * len(TRAIN_SIZES), 2 * len(VALID_SIZES))
