"""One rank of the two-rank data-parallel run with --train_norm (tests/test_train_norm_gpu.py): train.py's wiring as in
tests/train_audio_dp_worker.py — DataParallel + loss scaler + FusedAdamW on the HIP step — on a bf16 model, so that the kernels
read the norm weights' working copies, not their masters. Run as: python tests/train_norm_dp_worker.py <rank> <world> <port> <out_dir>."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flipped-vqa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

N_STEPS = 2
DTYPE = torch.bfloat16


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    multi = torch.cuda.device_count() >= world and os.environ.get("FVQA_DP_TEST_BACKEND", "auto") != "gloo"
    device_index = rank if multi else 0                       # (one GPU: both ranks share it over gloo, as tests/dp_worker.py)
    torch.cuda.set_device(device_index)
    if multi:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device_index))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import util.misc as misc
    from fvqa import synth
    from fvqa.optim import FusedAdamW, param_groups_weight_decay
    from fvqa.parallel import DataParallel
    from tests import train_norm_util as U
    from tests.dp_worker import batch_seed, perturb_trainables

    cfg = synth.preset("tiny", vaq=True, qav=True)
    model, args = U.build_model(cfg, DTYPE, device=f"cuda:{device_index}", train_norm=True)
    perturb_trainables(model, seed=1000 + rank)               # replicas start different, the norm masters included ...
    flat = model.flat_params()
    start = flat.flat.detach().cpu().clone()
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=0.01, betas=(0.9, 0.95), flat=flat)
    net = DataParallel(model)                                 # ... and leave here identical, working copies refreshed
    opt.grad_sync = net.sync_grads
    eng = model._engine
    trace = {"p_start": start, "p_init": flat.flat.detach().cpu().clone(), "names": list(flat.offsets),
             "numel": flat.flat.numel(), "work_init": eng.norm_work.detach().float().cpu().clone(),
             "norm_segments": {n: flat.offsets[n] for n in U.norm_names(model)}}
    scaler = misc.NativeScalerWithGradNormCount()
    for i in range(N_STEPS):
        opt.zero_grad()
        a, b, c = net(synth.make_batch(cfg, seed=batch_seed(rank, world, i)))
        scaler(a + b + c, opt, parameters=None, update_grad=True)
        torch.cuda.synchronize()
        trace[f"p{i}"] = flat.flat.detach().cpu().clone()
        trace[f"work{i}"] = eng.norm_work.detach().float().cpu().clone()
        trace[f"loss{i}"] = float((a + b + c).detach().sum())
    eng.check_gemm_error()
    torch.save(trace, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
