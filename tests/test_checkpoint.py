"""Checkpoint schema (utils.py:125-145) and state_dict key compatibility with the reference."""
import os

import torch

from oracle import restatement as R


def test_state_dict_keys_match_reference_layout():
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    assert set(ResNet(50, 32).state_dict()) == set(R.init_encoder_params(50, 32))
    assert list(RNN(16, 24, 30, 2).state_dict()) == list(R.init_decoder_params(16, 24, 30, 2, "gru"))
    assert list(RNN_LSTM(16, 24, 30, 2).state_dict()) == list(R.init_decoder_params(16, 24, 30, 2, "lstm"))
    want = set(R.init_decoder_params(16, 24, 30, 2, "gru", attn=dict(F=64, A=8)))
    assert set(RNN_Attn(16, 64, 8, 24, 30, 2).state_dict()) == want
    want = set(R.init_decoder_params(16, 24, 30, 2, "lstm", attn=dict(F=64, A=8)))
    assert set(RNN_Attn_LSTM(16, 64, 8, 24, 30, 2).state_dict()) == want
    # shapes of the keys the reference's golden vectors carry
    sd = RNN(64, 64, 50, 5).state_dict()
    from tests._util import load_fixture
    params, _, _ = load_fixture("gru_small.npz")
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}


def test_checkpoint_roundtrip(tmp_path):
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.utils import create_checkpoint, load_checkpoint
    cnn, rnn = ResNet(18, 16), RNN(16, 24, 30, 2)
    opt = torch.optim.SGD(list(rnn.parameters()), lr=0.1, momentum=0.9)
    path = create_checkpoint(cnn, rnn, opt, 3, 77, [1.5, 1.25], {"output_dir": str(tmp_path)})
    sd = torch.load(path, weights_only=True)
    assert set(sd) == {"encoder_state_dict", "decoder_state_dict", "optimizer_state_dict", "epoch", "step"}
    assert os.path.isfile(os.path.join(tmp_path, "model_3_metrics.ckpt"))
    cnn2, rnn2 = ResNet(18, 16), RNN(16, 24, 30, 2)
    assert load_checkpoint(path, cnn2, rnn2) == (3, 77)
    for k, v in rnn.state_dict().items():
        assert torch.equal(v, rnn2.state_dict()[k])
    for k, v in cnn.state_dict().items():
        assert torch.equal(v, cnn2.state_dict()[k])


def test_encoder_state_dict_saves_directly_once_flattened(tmp_path):
    """After the first forward the BatchNorm tensors are views into the engine's flat arrays (cnn._Backbone.flatten_bn, laid
    out here on the CPU as a forward lays them out on its device).  The reference's checkpoint code saves cnn.state_dict()
    as it stands, with no copy: torch.save must accept it (one storage is never viewed as two dtypes) and load it back."""
    from showtell_amd.cnn import ResNet
    cnn = ResNet(18, 16)
    cnn._bb.flatten_bn(torch.device("cpu"))
    cnn._bb.nbt.add_(3)
    with torch.no_grad():
        cnn._bb.flat["rv"].uniform_(0.5, 1.5)
    path = os.path.join(tmp_path, "enc.ckpt")
    torch.save({"encoder_state_dict": cnn.state_dict()}, path)
    back = torch.load(path, weights_only=True)["encoder_state_dict"]
    cnn2 = ResNet(18, 16)
    cnn2.load_state_dict(back)
    for k, v in cnn.state_dict().items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
        assert torch.equal(cnn2.state_dict()[k], v), k
    assert int(back["model.1.num_batches_tracked"]) == 3


def test_caption_word_format():
    from showtell_amd.utils import create_caption_word_format

    class V:
        index_to_word = {0: "<pad>", 1: "<start>", 2: "<end>", 3: "<unk>", 4: "a", 5: "dog"}
        word_to_index = {v: k for k, v in index_to_word.items()}
        def start_token(self): return "<start>"
        def end_token(self): return "<end>"
    assert create_caption_word_format([[1, 4, 5, 2, 4]], V()) == [["a", "dog"]]
    assert create_caption_word_format([[1, 4, 5, 2, 4]], V(), True) == [[["a", "dog"]]]
