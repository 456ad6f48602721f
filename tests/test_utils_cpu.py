"""Launch helpers, loggers, CIFAR data utilities, visualisation, compat packages, build."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from layer_wise_aaai20_amd.data import cifar as D
from layer_wise_aaai20_amd.utils import launch as L
from layer_wise_aaai20_amd.utils import logging as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_orders():
    assert L.build_ring_order([0, 1], [0, 1, 2]) == "0 1 2 3 4 5"
    assert L.get_skip_order(8) == [0, 3, 6, 1, 4, 7, 2, 5]
    assert L.get_skip_order(4) == [0, 2, 1, 3]
    r = L.get_rings(4, 8).split(" | ")
    assert len(r) == 4 and all(len(x.split()) == 32 for x in r)
    assert L.ring_env(1, 8) == {"NCCL_DEBUG": "VERSION"}


def test_text_encode_roundtrip_is_json():
    cfg = [{"ep": 0, "sz": 128, "bs": 512}, {"ep": [0, 5], "lr": [1.0, 2.0]}]
    assert L.text_decode(L.text_encode(cfg)) == cfg


def test_launch_local_propagates_exit_code(tmp_path):
    ok = L.launch_local(["-c", "import os,sys; sys.exit(0 if os.environ['WORLD_SIZE']=='2' else 3)"], 2)
    assert ok == 0
    bad = L.launch_local(["-c", "import os,sys; sys.exit(int(os.environ['RANK'])*7)"], 2)
    assert bad == 7


def test_timer_table_tsv(capsys):
    t = LG.Timer()
    assert t() >= 0 and t.total_time >= 0
    tl = LG.TableLogger()
    tl.append({"epoch": 1, "loss": np.float32(0.5)})
    assert "epoch" in capsys.readouterr().out
    tsv = LG.TSVLogger()
    tsv.append({"epoch": 1, "total time": 3600.0, "test acc": 0.9413})
    assert str(tsv).splitlines()[1] == "1\t1.00000000\t94.13"
    assert LG.PiecewiseLinear([0, 5, 24], [0, 0.4, 0])(2.5) == pytest.approx(0.2)


def test_stats_logger_single_sync():
    s = LG.StatsLogger(("loss", "correct"))
    s.append({"loss": torch.tensor([1.0, 3.0]), "correct": torch.tensor([True, False])})
    s.append({"loss": torch.tensor([2.0]), "correct": torch.tensor([True])})
    assert s.mean("loss") == pytest.approx(2.0) and s.mean("correct") == pytest.approx(2 / 3)


def test_file_and_tb_loggers(tmp_path):
    fl = LG.FileLogger(str(tmp_path), is_master=True, is_rank0=True)
    fl.event("hello")
    fl.verbose("v")
    tb = LG.TensorboardLogger(str(tmp_path))
    tb.log("times/step", 1.0)
    tb.update_step_count(10)
    tb.close()
    assert "hello" in open(tmp_path / "event.log").read()
    assert "times/step" in open(tmp_path / "scalars.jsonl").read()


def test_cifar_preprocessing_and_transform():
    x = np.random.randint(0, 256, (4, 32, 32, 3)).astype(np.uint8)
    p = D.pad(x, 4)
    assert p.shape == (4, 40, 40, 3)
    n = D.transpose(D.normalise(p))
    assert n.shape == (4, 3, 40, 40) and n.dtype == np.float32
    ds = list(zip(n, [0, 1, 2, 3]))
    tr = D.Transform(ds, [D.Crop(32, 32), D.FlipLR(), D.Cutout(8, 8)])
    tr.set_random_choices()
    img, lab = tr[0]
    assert img.shape == (3, 32, 32)


def test_gpu_batches_augment_cpu():
    data = torch.arange(2 * 3 * 40 * 40, dtype=torch.float32).reshape(2, 3, 40, 40)
    gb = D.GPUBatches(data, torch.tensor([0, 1]), 2, shuffle=False, augment=True, cutout=8)
    b = next(iter(gb))
    assert b["input"].shape == (2, 3, 32, 32)
    assert int((b["input"] == 0).sum()) >= 2 * 3 * 64 - 3   # an 8x8 cutout per image


def test_dot_graph_and_compat_imports():
    from CIFAR10 import core, torch_backend  # noqa: F401
    from IMAGENET.training import (dataloader, ddp, dist_utils, experimental_utils,  # noqa
                                   fp16util, logger, meter, resnet, sparsified_ddp,
                                   train_imagenet_nv)
    from layer_wise_aaai20_amd.models.cifar import resnet9
    from layer_wise_aaai20_amd.models.graph import Identity
    g = core.DotGraph(core.remove_by_type(resnet9(), Identity))
    src = g.dot_source()
    assert src.startswith("digraph") and "layer1_residual_res1_conv" in src
    assert core.cat(torch.ones(2), torch.zeros(1)).numel() == 3
    assert core.to_numpy(torch.ones(2)).sum() == 2


def test_bnwd_optim_params_keeps_all_params():
    from IMAGENET.training.experimental_utils import bnwd_optim_params
    from layer_wise_aaai20_amd.models.resnet import resnet18
    m = resnet18()
    gen = m.parameters()
    groups = bnwd_optim_params(m, gen, gen)       # the reference's fp32 call (D12)
    n = sum(len(g["params"]) for g in groups)
    assert n == len(list(m.parameters()))


def test_fp16_utils_roundtrip():
    from layer_wise_aaai20_amd.utils import fp16
    m = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4))
    h = fp16.network_to_half(m)
    assert h[1][0].weight.dtype == torch.float16 and h[1][1].weight.dtype == torch.float32
    mp, master = fp16.prep_param_lists(h)
    for p in mp:
        p.grad = torch.ones_like(p)
    fp16.model_grads_to_master_grads(mp, master)
    assert all(q.grad.dtype == torch.float32 for q in master)
    fp16.master_params_to_model_params(mp, master)


def test_extension_builds_for_gfx950():
    """`build()` must produce the in-tree .so bound to torch's HIP runtime (cross-compiled here)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    so = os.path.join(ROOT, "layer_wise_aaai20_amd", "_lwaaai_C.so")
    assert os.path.exists(so)
    needed = subprocess.run(["readelf", "-d", so], capture_output=True, text=True).stdout
    assert "libamdhip64.so.7" in needed
    import torch
    from layer_wise_aaai20_amd.ops import _ext
    ops = _ext.load(build_if_missing=False)
    assert ops.workspace_bytes(1, 1, 1) > 0


def test_launch_env_and_mpi_helpers(tmp_path):
    from layer_wise_aaai20_amd.utils import launch as L
    assert L.format_env_export(A=1, B="x") == "export A=1; export B=x"
    assert "NCCL_RINGS=" in L.get_nccl_params(2, 8)
    cmd = L.setup_mpi(["h1", "h2"], 8, path=str(tmp_path / "hosts.slots"), env={"K": "v"})
    assert (tmp_path / "hosts.slots").read_text() == "h1 slots=8\nh2 slots=8\n"
    assert cmd.startswith("mpirun -n 16 -N 8") and "-x K=v" in cmd
    assert L.run_parallel([lambda: 1, lambda: 2]) == [1, 2]
    (tmp_path / "d" / "train").mkdir(parents=True)
    (tmp_path / "d" / "validation").mkdir()
    assert L.mount_imagenet(str(tmp_path / "d")) == str(tmp_path / "d")
    import pytest
    with pytest.raises(FileNotFoundError):
        L.mount_imagenet(str(tmp_path))


def test_rank_device_mapping():
    """Rank → GPU binding of the CLIs: LOCAL_RANK when the launcher gives one, else
    rank % device_count (the reference binds every rank to cuda:0)."""
    from layer_wise_aaai20_amd.parallel.comm import rank_device_index
    assert [rank_device_index(r, 8) for r in range(8)] == list(range(8))
    assert [rank_device_index(r, 8) for r in range(8, 16)] == list(range(8))   # 2 nodes
    assert rank_device_index(13, 8, local_rank=5) == 5
    assert [rank_device_index(r, 2) for r in range(4)] == [0, 1, 0, 1]
    import pytest
    with pytest.raises(ValueError):
        rank_device_index(0, 0)


def test_env_local_rank(monkeypatch):
    from layer_wise_aaai20_amd.parallel import comm
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    monkeypatch.delenv("OMPI_COMM_WORLD_LOCAL_RANK", raising=False)
    assert comm.env_local_rank() is None
    monkeypatch.setenv("OMPI_COMM_WORLD_LOCAL_RANK", "3")
    assert comm.env_local_rank() == 3
    monkeypatch.setenv("LOCAL_RANK", "2")
    assert comm.env_local_rank() == 2
    # without a visible GPU a rank lands on the CPU (patched: the suite also runs on GPU hosts)
    monkeypatch.setattr(comm.torch.cuda, "is_available", lambda: False)
    assert comm.bind_rank_device(5).type == "cpu"


def test_ddp_rejects_single_process_multi_gpu():
    """Deliberate deviation (PARITY.md row 39): one process per GPU; the reference DDP's
    single-process replicate/scatter/gather mode (IMAGENET/training/ddp.py:207-219) is refused."""
    from torch import nn
    from layer_wise_aaai20_amd.parallel.ddp import DistributedDataParallel
    with pytest.raises(RuntimeError, match="one process per GPU"):
        DistributedDataParallel(nn.Linear(4, 4), device_ids=[0, 1])
    m = DistributedDataParallel(nn.Linear(4, 4), device_ids=[0])     # one device: fine
    assert m.engine.world == 1
