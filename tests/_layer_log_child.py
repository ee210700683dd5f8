"""Child process of tests/test_gpu_encoder_versions.py::test_executor_logs_what_the_planner_says:
    python tests/_layer_log_child.py <version> <bf16|f32> <B> <train 0|1> <log file> [<H> <W>]
One ResNet(version).backbone_features at H x W (224 x 224 if not given) with ST_LAYER_LOG set (the engine opens the log once per process)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(version, dtype, B, train, log, H=224, W=224):
    os.environ["ST_LAYER_LOG"] = log
    import torch
    from showtell_amd.cnn import ResNet
    torch.manual_seed(1)
    m = ResNet(int(version), 64, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32).cuda().train(bool(int(train)))
    x = torch.randn(int(B), 3, int(H), int(W), generator=torch.Generator().manual_seed(1))
    m.backbone_features(x.cuda())
    torch.cuda.synchronize()


if __name__ == "__main__":
    main(*sys.argv[1:])
