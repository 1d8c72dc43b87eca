"""Plain-torch restatement of the text-to-speech pieces (reference: adaptor/audio.py:327-336, 468-477, 721-763;
engine/criterion/tacotron2_loss.py:169-198; preprocessor/default/audio.py:442-476), used on the CPU and next to the GPU.
TEST INFRASTRUCTURE: torch's own ops in whatever dtype the inputs have (the tests pass float64 or float32), nothing of the kernels."""
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------- collation
def pack_frames(feature, n):
    if n == 1:
        return feature
    packed = feature.shape[0] // n
    return feature[: n * packed].reshape(packed, -1)


def collate(frames):
    """[L_i, F] frames -> (prev_outputs, target [B, Lmax, F], target_lengths int64 [B], ntokens)."""
    lmax = max(f.shape[0] for f in frames)
    target = frames[0].new_zeros((len(frames), lmax, frames[0].shape[1]))
    for i, f in enumerate(frames):
        target[i, : f.shape[0]] = f
    prev = torch.cat((target.new_zeros((len(frames), 1, target.shape[2])), target[:, :-1]), dim=1)
    lengths = torch.tensor([f.shape[0] for f in frames], dtype=torch.long)
    return prev, target, lengths, int(lengths.sum())


# ---------------------------------------------------------------------------------------------- time unfold / fold
def unfold1d(x, B, T, C, k):
    """x [B*T, C] -> col [B*T, ceil8(k*C)], taps (k, c), zero padding (k-1)/2 inside every sample: F.pad and index."""
    half = (k - 1) // 2
    xp = F.pad(x.view(B, T, C), (0, 0, half, half))                            # [B, T + k - 1, C]
    col = torch.stack([xp[:, j:j + T] for j in range(k)], dim=2).reshape(B * T, k * C)
    return F.pad(col, (0, (k * C + 7) // 8 * 8 - k * C))


# ---------------------------------------------------------------------------------------------- adaptor
def prenet(state, prefix, fbank):
    """prenet with dropout 0: layers of Linear + ReLU, then the projection to embed_dim."""
    x, i = fbank, 0
    while f"{prefix}prenet.0.layers.{i}.0.weight" in state:
        x = F.relu(F.linear(x, state[f"{prefix}prenet.0.layers.{i}.0.weight"], state[f"{prefix}prenet.0.layers.{i}.0.bias"]))
        i += 1
    return F.linear(x, state[f"{prefix}prenet.1.weight"], state[f"{prefix}prenet.1.bias"])


def conv1d_bn(x, w, b, gamma, beta, running_mean, running_var, training, eps=1e-5):
    """x [B, T, Cin] -> BatchNorm1d(Conv1d(x)) [B, T, Cout]; training: batch statistics over all B*T frames (biased variance)."""
    y = F.conv1d(x.transpose(1, 2), w, b, padding=(w.shape[2] - 1) // 2)
    y = F.batch_norm(y, None if training else running_mean, None if training else running_var, gamma, beta, training, 0.1, eps)
    return y.transpose(1, 2)


def postnet(state, prefix, x, training=True):
    i, layers = 0, []
    while f"{prefix}postnet.convolutions.{i}.0.weight" in state:
        layers.append(i)
        i += 1
    for i in layers:
        p = f"{prefix}postnet.convolutions.{i}."
        x = conv1d_bn(x, state[p + "0.weight"], state[p + "0.bias"], state[p + "1.weight"], state[p + "1.bias"],
                      state.get(p + "1.running_mean"), state.get(p + "1.running_var"), training)
        if i < layers[-1]:
            x = torch.tanh(x)
    return x


def head(state, prefix, x, training=True):
    """forward_output with dropout 0: the decoder's output x [B, T, D] -> (post, feature_out, eos_out [B, T, 1])."""
    feat = F.linear(x, state[prefix + "feat_proj.weight"], state[prefix + "feat_proj.bias"])
    eos = F.linear(x, state[prefix + "eos_proj.weight"], state[prefix + "eos_proj.bias"])
    return feat + postnet(state, prefix, feat, training), feat, eos


# ---------------------------------------------------------------------------------------------- criterion
def tacotron2_loss(feat, post, eos, target, lengths, pos_weight=1.0, reduction="mean"):
    """compute_loss of the reference criterion -> (loss, l1, mse, eos_loss), in the dtype of the inputs."""
    B, T, _ = target.shape
    mask = torch.arange(T, device=target.device)[None, :] < lengths[:, None]
    eos_tgt = (torch.arange(T, device=target.device)[None, :] == (lengths[:, None] - 1)).to(feat.dtype)
    _eos, _tgt_e = eos.reshape(B, T)[mask], eos_tgt[mask]
    _tgt, _feat, _post = target[mask], feat[mask], post[mask]
    l1 = F.l1_loss(_feat, _tgt, reduction=reduction) + F.l1_loss(_post, _tgt, reduction=reduction)
    mse = F.mse_loss(_feat, _tgt, reduction=reduction) + F.mse_loss(_post, _tgt, reduction=reduction)
    e = F.binary_cross_entropy_with_logits(_eos, _tgt_e, pos_weight=torch.tensor(pos_weight, dtype=feat.dtype, device=feat.device),
                                           reduction=reduction)
    return l1 + mse + e, l1, mse, e
