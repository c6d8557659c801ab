"""Drop-in proof for the reference's own harness: the reference's `Experiment.run_experiment_with_params`
(reference experiment.py:75-125) needs exactly two imports swapped —

    from model.model_factory import ModelFactory     ->  videocad_amd.model_factory
    from trainer import create_trainer               ->  videocad_amd.trainer

— and then drives them in this order: factory (constructor kwargs straight from the reference's JSON entry, a `"state_dict"` checkpoint
with its `module._orig_mod.` prefix stripped) -> optional torch.compile -> .to(device) -> create_trainer(packets, ..., model_type=, rank=)
-> train(epochs) -> evaluate(model) -> results.json.  This test makes the same calls, in the same order, with the same arguments, on a
two-batch synthetic loader with the kernels under the CPU emulator, and checks the numbers against the oracle.  (The harness's own Python is
not part of this repository, so the test restates its calls rather than importing it.)

What this pins: constructor kwargs straight from the reference's JSON entry (extra keys tolerated), `create_trainer` signature and
packets, `trainer.train(epochs)` returning the model, `trainer.evaluate(model)` returning a JSON-serialisable dict, the checkpoint the
trainer writes, and that a `torch.compile` wrapper around the model is harmless (the trainer drives the native module's engine; the
wrapper's forward is never traced).  The DDP branch (:94-109) needs CUDA (`device_ids=[0]`) and is covered by `trainer.unwrap` + the
GradSync gloo tests instead."""
import json
import os
import shutil

import pytest
import torch

import oputil as U
from oracle import restatement as O
from videocad_amd import synth
from videocad_amd.model_factory import ModelFactory
from videocad_amd.trainer import create_trainer

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("compile_flag", [False, True])
def test_reference_experiment_runs_on_videocad_amd(tmp_path, monkeypatch, compile_flag):
    monkeypatch.chdir(tmp_path)
    shutil.copy(os.path.join(HERE, "golden", "class_weights.json"), "class_weights.json")      # the trainer reads it CWD-relative (reference trainer.py:822)
    # the reference's JSON entry, depth-reduced so the emulator finishes in seconds (vit_depth is this build's test extension)
    params = dict(json.load(open(os.path.join(HERE, "golden", "model_configs.json")))["cad_past_10_actions_and_states_timestep_embedding"])
    params.update(num_decoder_layers=1, window_size=2, max_ep_len=8, vit_depth=1, compute_dtype="f32", dropout=0.0)
    ocfg = dict(O.CANONICAL_CONFIG); ocfg.update(vit_depth=1, num_decoder_layers=1, window_size=2, max_ep_len=8)
    batches = []
    for seed in (21, 22):
        b = synth.make_batch(1, 2, seed=seed)
        batches.append({k: (torch.from_numpy(v) if v is not None else None) for k, v in b.items()})
    pk = {"loader": batches, "sampler": None}
    tcfg = {"lr": 1e-5, "use_mse": True, "epochs": 1, "compile": compile_flag, "enable_parallel": False, "sequential": False,
            "save_frequency": 1, "val_frequency": 1, "early_stopping_enabled": False, "experiment_name": "dropin"}
    with U.emulated():
        # same initial weights as the oracle, through the harness's checkpoint path (experiment.py:61-71 `"state_dict": path`): a checkpoint
        # saved from a compiled, DDP-wrapped model, loaded and stripped of that prefix
        shapes = O.param_shapes(ocfg)
        weights = {k: synth.make_param(k, s) for k, s in shapes.items()}
        torch.save({"model_state_dict": {"module._orig_mod." + k: torch.from_numpy(v) for k, v in weights.items()}}, "init.pt")
        params["state_dict"] = "init.pt"
        sd = {k.replace("module._orig_mod.", ""): v for k, v in torch.load(params["state_dict"])["model_state_dict"].items()}
        model, model_type = ModelFactory().create_model(params["model_name"], params, "cpu", sd)
        if tcfg.get("compile", True):
            model = torch.compile(model, dynamic=False)
        model = model.to("cpu")
        trainer = create_trainer(pk, pk, pk, model, tcfg, "cpu", model_type=model_type, rank=0)
        model = trainer.train(tcfg["epochs"])
        res = trainer.evaluate(model)
    res = json.loads(json.dumps(res))                       # what the harness writes to results.json
    assert res["total_predictions"] > 0 and "cmd_accuracy" in res and "loss" in res
    assert os.path.exists(os.path.join("checkpoints", "dropin", "epoch_1.pt"))
    # the evaluation == the oracle's on the same two batches after the same two optimiser steps
    ot = O.OracleTrainer(weights, ocfg)
    for b in (21, 22):
        ot.step(synth.make_batch(1, 2, seed=b))
    tot = 0.0; correct = 0; total = 0
    for b in (21, 22):
        nb = synth.make_batch(1, 2, seed=b)
        with torch.no_grad():
            cmds, pars, tgt = ot.forward(nb)
            loss, m = O.compute_loss(cmds, pars, tgt)
        tot += float(loss); correct += m["correct_predictions"]; total += m["total_predictions"]
    assert abs(res["loss"] - tot / 2) < 1e-4 * abs(tot / 2), (res["loss"], tot / 2)
    assert res["correct_predictions"] == correct and res["total_predictions"] == total
