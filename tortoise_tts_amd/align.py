"""Redaction of [bracketed] prompt text (reference: tortoise/utils/wav2vec_alignment.py, Wav2VecAlignment.align / redact, applied to every
returned clip by tts() when enable_redaction is set).  Host side: the aligner's weight source, its configuration check, the CTC
tokenizer, the resampler's tap table and the alignment algorithm.  The model itself runs on the device (stages.AlignerStage,
csrc/align.hip); everything here works on the frame ids it returns.
"""
import glob
import json
import math
import os
from dataclasses import dataclass, field

import torch

ALIGNER_MODEL = "wav2vec2-large-robust-ft-libritts-voxpopuli"  # jbetker/... on the HF hub (wav2vec_alignment.py:52)
ALIGNER_TOKENIZER = "tacotron-symbols"                          # jbetker/tacotron-symbols (wav2vec_alignment.py:53)
SKIP = "~"
ORIG_SR, NEW_SR = 24000, 16000


# ----------------------------------------------------------------------------------------- weight source
def _hub_dirs():
    if os.environ.get("HF_HUB_CACHE"):
        return os.environ["HF_HUB_CACHE"]
    if os.environ.get("HF_HOME"):
        return os.path.join(os.environ["HF_HOME"], "hub")
    return os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub")


def _candidates(models_dir, name):
    out = []
    if models_dir:
        out.append(os.path.join(models_dir, name))
    out += sorted(glob.glob(os.path.join(_hub_dirs(), f"models--jbetker--{name}", "snapshots", "*")))
    return out


def _model_dir(models_dir):
    for d in _candidates(models_dir, ALIGNER_MODEL):
        if os.path.isfile(os.path.join(d, "config.json")) and any(
                os.path.isfile(os.path.join(d, f)) for f in ("model.safetensors", "pytorch_model.bin")):
            return d
    return None


def _tokenizer_dir(models_dir):
    for d in _candidates(models_dir, ALIGNER_TOKENIZER):
        if os.path.isfile(os.path.join(d, "vocab.json")):
            return d
    return None


def where_to_put_files(models_dir):
    return (f"put the HF-format files of jbetker/{ALIGNER_MODEL} (config.json + model.safetensors or pytorch_model.bin) in "
            f"{os.path.join(models_dir or '<models_dir>', ALIGNER_MODEL)} and those of jbetker/{ALIGNER_TOKENIZER} (vocab.json, "
            f"tokenizer_config.json) in {os.path.join(models_dir or '<models_dir>', ALIGNER_TOKENIZER)}, or in the Hugging Face hub cache")


def find_aligner(models_dir):
    """-> (config dict, state_dict, vocab dict, tokenizer config dict) read from disk, or None when the files are not there.  Looks in
    <models_dir>/<name>/ first, then in the HF hub cache snapshots ($HF_HUB_CACHE, else $HF_HOME/hub, else ~/.cache/huggingface/hub)."""
    md, td = _model_dir(models_dir), _tokenizer_dir(models_dir)
    if md is None or td is None:
        return None
    with open(os.path.join(md, "config.json")) as f:
        cfg = json.load(f)
    st = os.path.join(md, "model.safetensors")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    else:
        sd = torch.load(os.path.join(md, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    with open(os.path.join(td, "vocab.json")) as f:
        vocab = json.load(f)
    tok_cfg = {}
    for name in ("special_tokens_map.json", "tokenizer_config.json"):
        p = os.path.join(td, name)
        if os.path.isfile(p):
            with open(p) as f:
                tok_cfg.update({k: v for k, v in json.load(f).items() if isinstance(v, (str, bool, int, float))})
    return cfg, sd, vocab, tok_cfg


# transformers.Wav2Vec2Config's defaults: what a config.json that omits a key describes
HF_DEFAULTS = dict(feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False, hidden_act="gelu", feat_extract_activation="gelu",
                   hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, conv_dim=[512] * 7,
                   conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], num_conv_pos_embeddings=128,
                   num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, vocab_size=32, use_weighted_layer_sum=False, add_adapter=False)


def check_config(cfg):
    """The configuration the reference's checkpoint has - the only one the device stage implements; a key config.json omits takes
    Wav2Vec2Config's default.  ValueError naming the field otherwise.  -> the tt_w2v_config fields."""
    def get(k):
        return cfg.get(k, HF_DEFAULTS[k])

    want = {"feat_extract_norm": "layer", "do_stable_layer_norm": True, "conv_bias": True, "hidden_act": "gelu",
            "feat_extract_activation": "gelu", "use_weighted_layer_sum": False, "add_adapter": False}
    for k, v in want.items():
        if get(k) != v:
            raise ValueError(f"wav2vec2 aligner config: {k}={get(k)!r} is not supported (the reference's checkpoint has {v!r})")
    try:
        D, H = int(get("hidden_size")), int(get("num_attention_heads"))
        layers, ff, vocab = int(get("num_hidden_layers")), int(get("intermediate_size")), int(get("vocab_size"))
        groups, pk, eps = int(get("num_conv_pos_embedding_groups")), int(get("num_conv_pos_embeddings")), float(get("layer_norm_eps"))
    except (TypeError, ValueError) as ex:
        raise ValueError(f"wav2vec2 aligner config: a size field is not a number ({ex})") from None
    if D != 64 * H:
        raise ValueError(f"wav2vec2 aligner config: num_attention_heads={H} with hidden_size={D} is not 64-wide heads")
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        v = get(k)
        if not isinstance(v, (list, tuple)) or len(v) != 7 or not all(isinstance(x, int) and x >= 1 for x in v):
            raise ValueError(f"wav2vec2 aligner config: {k}={v!r} is not 7 positive integers (the 7-layer feature encoder)")
    conv_dim, kern, stride = list(get("conv_dim")), list(get("conv_kernel")), list(get("conv_stride"))
    if any(c != 512 for c in conv_dim):
        raise ValueError(f"wav2vec2 aligner config: conv_dim={conv_dim} is not 512 channels in every feature-encoder layer")
    if kern[0] != 10 or any(s > k + 1 for k, s in zip(kern[1:], stride[1:])):
        raise ValueError(f"wav2vec2 aligner config: conv_kernel={kern} / conv_stride={stride} is not supported (a first kernel of 10, "
                         f"strides at most kernel + 1)")
    if D % groups or (D // groups) % 64:
        raise ValueError(f"wav2vec2 aligner config: num_conv_pos_embedding_groups={groups} with hidden_size={D} is not 64-channel groups")
    if pk % 2 or pk < 2:
        raise ValueError(f"wav2vec2 aligner config: num_conv_pos_embeddings={pk} is not an even kernel")
    return dict(dim=D, heads=H, layers=layers, ff_dim=ff, conv_dim=512, conv_kernel=kern, conv_stride=stride, pos_kernel=pk, pos_groups=groups,
                vocab=vocab, eps=eps)


def fold_pos_conv(sd, prefix="wav2vec2.encoder.pos_conv_embed.conv."):
    """The positional conv's weight norm (weight_norm(dim=2)) folded into one plain weight: older checkpoints store weight_g / weight_v,
    transformers 5.x parametrizations.weight.original0 / original1."""
    if prefix + "weight" in sd:
        return sd[prefix + "weight"].float()
    for g_key, v_key in (("weight_g", "weight_v"), ("parametrizations.weight.original0", "parametrizations.weight.original1")):
        if prefix + g_key in sd:
            g, v = sd[prefix + g_key].float(), sd[prefix + v_key].float()
            return v * (g / v.norm(dim=(0, 1), keepdim=True))
    raise KeyError(f"{prefix}weight (or its weight-norm pair) is missing from the aligner's state_dict")


# ----------------------------------------------------------------------------------------- CTC tokenizer
class CtcTokenizer:
    """What wav2vec_alignment.py uses of transformers.Wav2Vec2CTCTokenizer: encode (one id per character, ' ' -> the word delimiter, unknown
    -> unk) and decode (CTC grouping, blanks dropped, delimiter -> ' ', clean_up_tokenization_spaces as tokenizer_config.json says; True,
    the default of the transformers release the reference ran under, when it does not say)."""

    def __init__(self, vocab, config=None):
        c = dict(config or {})
        self.encoder = dict(vocab)
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.pad, self.unk = c.get("pad_token", "<pad>"), c.get("unk_token", "<unk>")
        self.delim = c.get("word_delimiter_token", "|")
        self.do_lower_case = bool(c.get("do_lower_case", False))
        self.cleanup = bool(c.get("clean_up_tokenization_spaces", True))

    def encode(self, text):
        if self.do_lower_case:
            text = text.upper()
        unk = self.encoder.get(self.unk)
        return [self.encoder.get(ch, unk) for ch in text.replace(" ", self.delim)]

    def decode(self, ids):
        toks = [self.decoder.get(int(i), self.unk) for i in ids]
        chars = [t for j, t in enumerate(toks) if j == 0 or t != toks[j - 1]]
        chars = [" " if t == self.delim else t for t in chars if t != self.pad]
        s = "".join(chars).strip()
        if self.do_lower_case:
            s = s.lower()
        if self.cleanup:
            s = (s.replace(" .", ".").replace(" ?", "?").replace(" !", "!").replace(" ,", ",").replace(" ' ", "'").replace(" n't", "n't")
                 .replace(" 'm", "'m").replace(" 's", "'s").replace(" 've", "'ve").replace(" 're", "'re"))
        return s


# ----------------------------------------------------------------------------------------- resampler
def resample_taps():
    """torchaudio.functional.resample(x, 24000, 16000) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), reduced by
    the gcd to 3 -> 2: the [2][23] float32 kernel of _get_sinc_resample_kernel, computed with its formula in float32 (the waveform's dtype)."""
    orig, new, lw = 3, 2, 6
    base = min(orig, new) * 0.99
    width = math.ceil(lw * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float32)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float32)[:, None, None] / new + idx
    t *= base
    t = t.clamp_(-lw, lw)
    window = torch.cos(t * math.pi / lw / 2) ** 2
    t *= math.pi
    kern = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kern *= window * (base / orig)
    return kern.reshape(new, -1)


def resampled_length(S):
    return (2 * S + 2) // 3  # ceil(new * S / orig)


def frames_for(samples, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2)):
    """Frames the model produces for a 24 kHz clip (0: shorter than the receptive field)."""
    n = resampled_length(samples)
    for k, s in zip(conv_kernel, conv_stride):
        n = (n - k) // s + 1 if n >= k else 0
    return n


# ----------------------------------------------------------------------------------------- alignment
def max_alignment(s1, s2, skip=SKIP):
    """wav2vec_alignment.py max_alignment, restated as an iterative dynamic programme over suffix pairs (the reference recurses once per
    character and reaches Python's recursion limit on long texts).  Same result, tie-break included: dropping a character of s2 wins only
    when it keeps strictly more characters of s1."""
    if skip in s1:
        raise ValueError(f"the text contains the alignment's skip character {skip!r}")
    n1, n2 = len(s1), len(s2)
    # score[i][j]: characters of s1[i:] kept by the alignment of s1[i:] with s2[j:]; eq[i][j]: s1[i:] == s2[j:]
    score = [[0] * (n2 + 1) for _ in range(n1 + 1)]
    eq = [[False] * (n2 + 1) for _ in range(n1 + 1)]
    eq[n1][n2] = True
    for i in range(n1 - 1, -1, -1):
        a = n1 - i
        row, nrow, erow, enrow = score[i], score[i + 1], eq[i], eq[i + 1]
        for j in range(n2 - 1, -1, -1):
            if s1[i] == s2[j]:
                erow[j] = enrow[j + 1] and a == n2 - j
                row[j] = a if erow[j] else 1 + nrow[j + 1]
            else:
                sa, sb = row[j + 1], nrow[j]
                row[j] = sa if sa > sb else sb
    out, i, j = [], 0, 0
    while i < n1:
        if j == n2:
            out.append(skip * (n1 - i))
            break
        if eq[i][j]:
            out.append(s1[i:])
            break
        if s1[i] == s2[j]:
            out.append(s1[i])
            i, j = i + 1, j + 1
        elif score[i][j + 1] > score[i + 1][j]:
            j += 1
        else:
            out.append(skip)
            i += 1
    return "".join(out)


def alignments_from_frames(frame_ids, tokenizer, text, samples):
    """Wav2VecAlignment.align after the model: the frame ids (argmax of every frame's logits) of a clip of `samples` 24 kHz samples and the
    text it speaks -> the sample index where every character of `text` starts.  RuntimeError where the reference asserts."""
    ids = [int(t) for t in frame_ids]
    pred = tokenizer.decode(ids)
    fixed = max_alignment(text.lower(), pred)
    comp = samples // len(ids)
    toks, chars = tokenizer.encode(fixed), list(fixed)
    if len(toks) == 1:
        return [0]  # "The alignment is simple; there is only one token."
    toks.pop(0)
    chars.pop(0)
    al = [0]

    def pop_till_you_win():
        if not toks:
            return None
        tok, ch = toks.pop(0), chars.pop(0)
        while ch == SKIP:
            al.append(-1)
            if not toks:
                return None
            tok, ch = toks.pop(0), chars.pop(0)
        return tok

    nxt = pop_till_you_win()
    for i, top in enumerate(ids):
        if nxt == top:
            al.append(i * comp)
            if toks:
                nxt = pop_till_you_win()
            else:
                break
    pop_till_you_win()
    if not (len(toks) == 0 and len(al) == len(text)):
        raise RuntimeError(f"redaction: could not align the text with the audio ({len(al)} of {len(text)} characters placed; the aligner "
                           f"heard {pred!r})")
    al.append(samples)
    for i in range(len(al)):
        if al[i] == -1:
            nf = next(j for j in range(i + 1, len(al)) if al[j] != -1)
            for j in range(i, nf):
                al[j] = (j - i + 1) * (al[nf] - al[i - 1]) // (nf - i + 1) + al[i - 1]
    return al[:-1]


def redaction_plan(text):
    """Wav2VecAlignment.redact's text side -> (the bare text the aligner is given, the kept (start, stop) character intervals), or None for
    text without '['.  ValueError for an unpaired '[' and for text with nothing left to keep."""
    if "[" not in text:
        return None
    parts = text.split("[")
    full = [parts[0]]
    for p in parts[1:]:
        if "]" not in p:
            raise ValueError('redaction: every "[" must be paired with a "]" with no nesting')
        full.extend(p.split("]"))
    keep, last = [], 0
    for i, part in enumerate(full):
        if i % 2 == 0 and part != "":
            keep.append((last, max(0, last + len(part) - 1)))
        last += len(part)
    if not keep:
        raise ValueError("redaction: the whole text is [bracketed], nothing would be left to speak")
    return "".join(full), keep


def redact(audio, text, frame_ids_fn, tokenizer):
    """Wav2VecAlignment.redact: audio [1, S] at 24 kHz (any device) -> the clip with the [bracketed] passages cut out.  frame_ids_fn(audio)
    returns the model's frame ids of the clip."""
    plan = redaction_plan(text)
    if plan is None:
        return audio
    bare, keep = plan
    S = audio.shape[-1]
    al = alignments_from_frames(frame_ids_fn(audio), tokenizer, bare, S)
    return torch.cat([audio[:, al[a]:al[b]] for a, b in keep], dim=-1)


# ----------------------------------------------------------------------------------------- forced alignment (word timings)
# The CTC Viterbi alignment of the text with the model's logits (stages.CtcAlignStage, csrc/ctc_align.hip) gives every character of the text
# a first and a last frame and a confidence.  What follows is its host side: text -> target ids, frames -> samples, characters -> words.
# The text is taken as it is spoken: numbers and abbreviations are NOT expanded here ("23" has no alignable character); callers pass
# spoken-form text.
class AlignmentTargets:
    """ids: the CTC target; chars: its characters as the text has them (' ' for the word delimiter); index[i]: the target position text[i]
    belongs to - its own when the character is part of the target, else that of the last kept character before it (-1: none)."""

    def __init__(self, text, ids, chars, index, kept):
        self.text, self.ids, self.chars, self.index, self.kept = text, ids, chars, index, kept


def blank_id(tokenizer):
    return tokenizer.encoder[tokenizer.pad]


def alignment_targets(text, tokenizer):
    """The text as the aligner's CTC target: case as the tokenizer has it, spaces -> the word delimiter (runs collapse, none at either end),
    characters outside the vocabulary (punctuation the model does not spell, digits) dropped."""
    cased = text.upper() if tokenizer.do_lower_case else text
    enc, special = tokenizer.encoder, {tokenizer.pad, tokenizer.unk}
    delim = enc.get(tokenizer.delim)
    ids, chars, index, kept = [], [], [], []
    for ch, orig in zip(cased, text):
        tok = None
        if ch.isspace():
            if delim is not None and ids and ids[-1] != delim:
                tok = delim
                orig = " "
        elif ch in enc and ch not in special and ch != tokenizer.delim:
            tok = enc[ch]
        if tok is not None:
            ids.append(tok)
            chars.append(orig)
        kept.append(tok is not None)
        index.append(len(ids) - 1)
    if ids and ids[-1] == delim:  # a trailing delimiter: its text position falls back to the character before it
        ids.pop()
        chars.pop()
        last = len(ids) - 1
        for i in range(len(index)):
            if index[i] > last:
                index[i], kept[i] = last, False
    return AlignmentTargets(text, ids, chars, index, kept)


def frame_samples(fields):
    """24 kHz samples one frame of the model covers: the feature encoder's total stride at 16 kHz, times 3 / 2."""
    return math.prod(fields["conv_stride"]) * ORIG_SR // NEW_SR


@dataclass
class Alignment:
    """Where a text is spoken in a clip of `samples` 24 kHz samples.  chars: (character, start_sample, end_sample, confidence) of every
    character of the CTC target (' ' between words); words: (word, start_sample, end_sample, confidence) of every whitespace-separated word
    of the text, confidence = the minimum over its characters (NaN and an empty span for a word with no alignable character).  Frames the
    path spends in blanks belong to nobody: they are the pauses.  score: the path's log-probability."""
    text: str
    chars: list
    words: list
    score: float
    samples: int
    index: list = field(default_factory=list)  # text position -> position in chars (AlignmentTargets.index)
    kept: list = field(default_factory=list)
    rate: int = ORIG_SR  # samples per second of the clip the positions count (another one after a sample-rate conversion)

    def seconds(self, rate=None):
        """words with their times in seconds: (word, start_s, end_s, confidence)."""
        rate = self.rate if rate is None else rate
        return [(w, a / rate, b / rate, c) for w, a, b, c in self.words]

    def char_start(self, i):
        """Sample where text[i] starts; a character that is not part of the target sits at the end of the last one before it that is."""
        j = self.index[i]
        return 0 if j < 0 else self.chars[j][1] if self.kept[i] else self.chars[j][2]

    def char_end(self, i):
        j = self.index[i]
        return 0 if j < 0 else self.chars[j][2]

    def to_srt(self, max_chars=42, rate=None):
        """SubRip cues of at most max_chars characters, cut on word boundaries (a longer single word gets a cue of its own)."""
        rate = self.rate if rate is None else rate

        def stamp(n):
            ms = (n * 1000 + rate // 2) // rate
            return "%02d:%02d:%02d,%03d" % (ms // 3600000, ms // 60000 % 60, ms // 1000 % 60, ms % 1000)

        cues, cur = [], []
        for w in self.words:
            if cur and len(" ".join(x[0] for x in cur)) + 1 + len(w[0]) > max_chars:
                cues.append(cur)
                cur = []
            cur.append(w)
        if cur:
            cues.append(cur)
        return "".join("%d\n%s --> %s\n%s\n\n" % (n + 1, stamp(c[0][1]), stamp(c[-1][2]), " ".join(x[0] for x in c)) for n, c in enumerate(cues))


def build_alignment(targets, spans, conf, score, samples, frame_len):
    """AlignmentTargets + the device's spans [L][2] (first, last frame) and conf [L] -> Alignment.  start = first * frame_len,
    end = min(samples, (last + 1) * frame_len)."""
    chars = [(ch, int(a) * frame_len, min(samples, (int(b) + 1) * frame_len), float(c)) for ch, (a, b), c in zip(targets.chars, spans, conf)]
    words, text, i, prev_end = [], targets.text, 0, 0
    while i < len(text):
        if text[i].isspace():
            i += 1
            continue
        j = i
        while j < len(text) and not text[j].isspace():
            j += 1
        own = [chars[targets.index[p]] for p in range(i, j) if targets.kept[p]]
        if own:
            words.append((text[i:j], own[0][1], own[-1][2], min(c[3] for c in own)))
            prev_end = own[-1][2]
        else:
            words.append((text[i:j], prev_end, prev_end, float("nan")))
        i = j
    return Alignment(text, chars, words, float(score), int(samples), list(targets.index), list(targets.kept))


def resample_alignment(al, to_rate, n_out):
    """An alignment of a clip at al.rate -> the same alignment of that clip converted to `to_rate` Hz, n_out samples long: every position
    goes through resample.map_sample, s -> min(n_out, (s Q + P / 2) / P) with P / Q = al.rate / to_rate."""
    from . import resample as rs
    P, Q = rs.ratio(al.rate, to_rate)
    f = lambda s_: rs.map_sample(s_, P, Q, n_out)
    return Alignment(al.text, [(c, f(a), f(b), p) for c, a, b, p in al.chars], [(w, f(a), f(b), p) for w, a, b, p in al.words], al.score,
                     int(n_out), list(al.index), list(al.kept), int(to_rate))


def empty_alignment(targets, samples):
    """The alignment of a text with nothing alignable: no characters, every word an empty span at 0."""
    return build_alignment(targets, [], [], 0.0, samples, 1)


def redact_forced(audio, text, align_fn):
    """redact() with the forced alignment: audio [1, S] -> the concatenation of the kept passages, each cut from the start of its first
    character to the end of its last.  align_fn(audio, bare text) -> Alignment."""
    plan = redaction_plan(text)
    if plan is None:
        return audio
    bare, keep = plan
    al = align_fn(audio, bare)
    return torch.cat([audio[:, al.char_start(a):al.char_end(b)] for a, b in keep], dim=-1)  # (keep: first and last character, inclusive)
