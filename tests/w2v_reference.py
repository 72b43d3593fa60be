"""TEST INFRASTRUCTURE ONLY - the reference's redaction path transcribed for the tests: torchaudio's 24 -> 16 kHz resample
(_get_sinc_resample_kernel / _apply_sinc_resample_kernel with their defaults), Wav2VecAlignment.align / redact / max_alignment as
tortoise/utils/wav2vec_alignment.py (v3.0) writes them, recursion and asserts included, and a seeded transformers.Wav2Vec2ForCTC with the
reference checkpoint's architecture."""
import math

import torch

# a tacotron-symbols-like CTC vocabulary: blank / specials, the word delimiter, letters, punctuation
VOCAB = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4}
for _c in "abcdefghijklmnopqrstuvwxyz'.,?!-":
    VOCAB[_c] = len(VOCAB)
TOK_CFG = {"pad_token": "<pad>", "unk_token": "<unk>", "bos_token": "<s>", "eos_token": "</s>", "word_delimiter_token": "|",
           "do_lower_case": False}


def hf_tokenizer(tmpdir, clean_up=True):
    import json
    import os
    from transformers import Wav2Vec2CTCTokenizer
    p = os.path.join(str(tmpdir), "vocab.json")
    with open(p, "w") as f:
        json.dump(VOCAB, f)
    return Wav2Vec2CTCTokenizer(p, clean_up_tokenization_spaces=clean_up, **{k: v for k, v in TOK_CFG.items()})


def large_config(**over):
    """The reference checkpoint's architecture (wav2vec2-large-robust: 24 x 1024, 16 heads, stable layer norm) with this vocabulary."""
    cfg = dict(vocab_size=len(VOCAB), hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
               feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, hidden_act="gelu", feat_extract_activation="gelu",
               conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128,
               num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, pad_token_id=0, hidden_dropout=0.0, attention_dropout=0.0,
               activation_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0)
    cfg.update(over)
    return cfg


def small_config(**over):
    return large_config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, num_conv_pos_embeddings=16,
                        num_conv_pos_embedding_groups=2, **over)


def hf_model(cfg, seed=0):
    """Wav2Vec2ForCTC with seeded random weights (every parameter of the default init, then the norms and biases perturbed so that they
    are not the identity); the special tokens other than the blank never win a frame, as in a trained CTC head."""
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    torch.manual_seed(seed)
    m = Wav2Vec2ForCTC(Wav2Vec2Config(**cfg)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias") or "layer_norm" in name:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
        m.lm_head.weight.mul_(8.0)
        m.lm_head.bias[1:4] -= 100.0
    m.config._attn_implementation = "eager"
    return m


def sinc_resample_kernel(dtype=torch.float32):
    orig, new, lw, rolloff = 3, 2, 6, 0.99
    base = min(orig, new) * rolloff
    width = math.ceil(lw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=dtype)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=dtype)[:, None, None] / new + idx
    t *= base
    t = t.clamp_(-lw, lw)
    window = torch.cos(t * math.pi / lw / 2) ** 2
    t *= math.pi
    scale = base / orig
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    return kernels, width  # [new, 1, 23]


def resample(waveform):
    """torchaudio.functional.resample(waveform [..., S], 24000, 16000)."""
    kernel, width = sinc_resample_kernel(waveform.dtype)
    kernel = kernel.to(waveform.device)
    shape = waveform.size()
    waveform = waveform.view(-1, shape[-1])
    num_wavs, length = waveform.shape
    waveform = torch.nn.functional.pad(waveform, (width, width + 3))
    resampled = torch.nn.functional.conv1d(waveform[:, None], kernel, stride=3)
    resampled = resampled.transpose(1, 2).reshape(num_wavs, -1)
    target_length = torch.ceil(torch.as_tensor(2 * length / 3)).long()
    resampled = resampled[..., :target_length]
    return resampled.view(shape[:-1] + resampled.shape[-1:])


def model_logits(model, audio):
    """wav2vec_alignment.py:65-70 -> logits [T, V] of a clip [1, S] at 24 kHz."""
    with torch.no_grad():
        x = resample(audio)
        clip_norm = (x - x.mean()) / torch.sqrt(x.var() + 1e-7)
        return model(clip_norm).logits[0]


def max_alignment(s1, s2, skip_character='~', record=None):
    if record is None:
        record = {}
    assert skip_character not in s1, f"Found the skip character {skip_character} in the provided string, {s1}"
    if len(s1) == 0:
        return ''
    if len(s2) == 0:
        return skip_character * len(s1)
    if s1 == s2:
        return s1
    if s1[0] == s2[0]:
        return s1[0] + max_alignment(s1[1:], s2[1:], skip_character, record)
    take_s1_key = (len(s1), len(s2) - 1)
    if take_s1_key in record:
        take_s1, take_s1_score = record[take_s1_key]
    else:
        take_s1 = max_alignment(s1, s2[1:], skip_character, record)
        take_s1_score = len(take_s1.replace(skip_character, ''))
        record[take_s1_key] = (take_s1, take_s1_score)
    take_s2_key = (len(s1) - 1, len(s2))
    if take_s2_key in record:
        take_s2, take_s2_score = record[take_s2_key]
    else:
        take_s2 = max_alignment(s1[1:], s2, skip_character, record)
        take_s2_score = len(take_s2.replace(skip_character, ''))
        record[take_s2_key] = (take_s2, take_s2_score)
    return take_s1 if take_s1_score > take_s2_score else skip_character + take_s2


def align_from_logits(logits, tokenizer, expected_text, orig_len):
    """Wav2VecAlignment.align after `logits = self.model(clip_norm).logits` (v3.0); logits [T, V] (or the argmax ids [T] as a tensor)."""
    pred_ids = logits.argmax(-1) if logits.dim() == 2 else logits
    pred_string = tokenizer.decode(pred_ids.tolist())
    fixed_expectation = max_alignment(expected_text.lower(), pred_string)
    w2v_compression = orig_len // pred_ids.shape[0]
    expected_tokens = tokenizer.encode(fixed_expectation)
    expected_chars = list(fixed_expectation)
    if len(expected_tokens) == 1:
        return [0]
    expected_tokens.pop(0)
    expected_chars.pop(0)
    alignments = [0]

    def pop_till_you_win():
        if len(expected_tokens) == 0:
            return None
        popped = expected_tokens.pop(0)
        popped_char = expected_chars.pop(0)
        while popped_char == '~':
            alignments.append(-1)
            if len(expected_tokens) == 0:
                return None
            popped = expected_tokens.pop(0)
            popped_char = expected_chars.pop(0)
        return popped

    next_expected_token = pop_till_you_win()
    for i, top in enumerate(pred_ids):
        if next_expected_token == top:
            alignments.append(i * w2v_compression)
            if len(expected_tokens) > 0:
                next_expected_token = pop_till_you_win()
            else:
                break
    pop_till_you_win()
    if not (len(expected_tokens) == 0 and len(alignments) == len(expected_text)):
        assert False, "alignment failed"
    alignments.append(orig_len)
    for i in range(len(alignments)):
        if alignments[i] == -1:
            for j in range(i + 1, len(alignments)):
                if alignments[j] != -1:
                    next_found_token = j
                    break
            for j in range(i, next_found_token):
                gap = alignments[next_found_token] - alignments[i - 1]
                alignments[j] = (j - i + 1) * gap // (next_found_token - i + 1) + alignments[i - 1]
    return alignments[:-1]


def redact(audio, expected_text, logits_fn, tokenizer):
    """Wav2VecAlignment.redact; logits_fn(audio) -> logits [T, V] (or argmax ids [T])."""
    if '[' not in expected_text:
        return audio
    splitted = expected_text.split('[')
    fully_split = [splitted[0]]
    for spl in splitted[1:]:
        assert ']' in spl, 'Every "[" character must be paired with a "]" with no nesting.'
        fully_split.extend(spl.split(']'))
    non_redacted_intervals = []
    last_point = 0
    for i in range(len(fully_split)):
        if i % 2 == 0 and fully_split[i] != "":
            end_interval = max(0, last_point + len(fully_split[i]) - 1)
            non_redacted_intervals.append((last_point, end_interval))
        last_point += len(fully_split[i])
    bare_text = ''.join(fully_split)
    alignments = align_from_logits(logits_fn(audio), tokenizer, bare_text, audio.shape[-1])
    output_audio = []
    for nri in non_redacted_intervals:
        start, stop = nri
        output_audio.append(audio[:, alignments[start]:alignments[stop]])
    return torch.cat(output_audio, dim=-1)


def test_clip(seconds, seed=0, sr=24000):
    """A deterministic 24 kHz clip [1, S]: a few drifting tones with noise, |x| < 1."""
    g = torch.Generator().manual_seed(seed)
    S = int(round(seconds * sr))
    t = torch.arange(S, dtype=torch.float64) / sr
    x = sum(0.15 * torch.sin(2 * math.pi * (f + 40 * torch.sin(2 * math.pi * 0.7 * t)) * t) for f in (180.0, 420.0, 1150.0))
    x = x + 0.05 * torch.randn(S, generator=g, dtype=torch.float64)
    return x.float().reshape(1, S)


def text_from_prediction(pred):
    """A bracketed text the clip's own decoded prediction aligns with: the first third of it in brackets."""
    n = len(pred)
    return "[" + pred[: n // 3] + "]" + pred[n // 3:]
