"""No GPU: the chunk rule of long prompts (75-token chunks cut at words, empty chunks up to the run's count, the 225-token limit),
token positions in the concatenated chunks, the argument checks of tmix_xattn_token_maps_long (the library loads without a GPU), the
sampler's position limit and the CLI flags."""
import ctypes as C
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_WORD = "photorealistic"          # 10 tokens in the fixture vocabulary


@pytest.fixture(scope="module")
def tok(golden_dir):
    from tweediemix_amd import text as T
    return T.ClipBPETokenizer.from_pretrained(os.path.join(golden_dir, "clip_tok"))


def _ids(tok, words):
    return [tok.convert_tokens_to_ids(t) for t in tok.tokenize(" ".join(words))]


# ------------------------------------------------------------------------------------------------ 1. chunking
def test_eighty_one_token_words_give_chunks_of_75_and_5(tok):
    from tweediemix_amd import text as T
    prompt = " ".join(["cat"] * 80)
    assert len(tok.tokenize(prompt)) == 80
    chunks = T.chunk_prompt(tok, prompt)
    assert [len(tok.tokenize(c)) for c in chunks] == [75, 5]
    (ids,), c = T.long_ids(tok, [prompt])
    assert c == 2 and ids.shape == (1, 2, 77)
    cat, bos, eos, pad = tok.convert_tokens_to_ids("cat</w>"), tok.bos_token_id, tok.eos_token_id, tok.pad_token_id
    assert ids[0, 0].tolist() == [bos] + [cat] * 75 + [eos]
    assert ids[0, 1].tolist() == [bos] + [cat] * 5 + [eos] + [pad] * 70
    assert torch.equal(ids[0], tok(chunks))                               # a chunk is what __call__ makes of its text


def test_multi_token_word_at_slot_74_moves_whole_to_the_next_chunk(tok):
    from tweediemix_amd import text as T
    n_long = len(tok.tokenize(LONG_WORD))
    assert n_long > 2
    words = ["cat"] * 73 + [LONG_WORD, "dog"]                             # the long word would take slots 74 .. 74 + n - 1 of chunk 1
    chunks = T.chunk_prompt(tok, " ".join(words))
    assert chunks == [" ".join(["cat"] * 73), LONG_WORD + " dog"]
    (ids,), c = T.long_ids(tok, [" ".join(words)])
    assert c == 2
    assert ids[0, 0, 74].item() == tok.eos_token_id and ids[0, 0, 75].item() == tok.pad_token_id      # two slots stay unused
    assert ids[0, 1, 1:1 + n_long + 1].tolist() == _ids(tok, [LONG_WORD, "dog"])
    # all tokens of the prompt survive, in order
    flat = [i for ch in chunks for i in _ids(tok, [ch])]
    assert flat == _ids(tok, words)


def test_one_chunk_prompt_gives_the_tokenizers_own_ids(tok, golden_dir):
    from tweediemix_amd import text as T
    tok2 = T.ClipBPETokenizer.from_pretrained(os.path.join(golden_dir, "clip_tok"))
    tok2.pad_token = "!"                                                   # tokenizer_2 of the SDXL checkpoint
    for prompt in ("photo of a cat and a dog running, mountain background", "a cat's   Photo!!  12 dogs", ""):
        ids, c = T.long_ids([tok, tok2], [prompt])
        assert c == 1
        assert torch.equal(ids[0][:, 0], tok([prompt])) and torch.equal(ids[1][:, 0], tok2([prompt]))
    tok.add_tokens("<new1>")
    ids, c = T.long_ids(tok, ["photo of a <new1> cat"])
    assert c == 1 and torch.equal(ids[0][:, 0], tok(["photo of a <new1> cat"]))
    assert tok.convert_tokens_to_ids("<new1>") in ids[0][0, 0].tolist()


def test_rows_of_unequal_length_are_padded_with_empty_chunks(tok):
    from tweediemix_amd import text as T
    prompts = [" ".join(["cat"] * 80), "a dog", " ".join(["dog"] * 160)]
    assert T.run_chunks(tok, prompts) == 3
    (ids,), c = T.long_ids(tok, prompts)
    assert c == 3 and ids.shape == (3, 3, 77)
    empty = tok([""])[0]
    assert empty.tolist() == [tok.bos_token_id, tok.eos_token_id] + [tok.pad_token_id] * 75
    assert torch.equal(ids[0, 2], empty) and torch.equal(ids[1, 1], empty) and torch.equal(ids[1, 2], empty)
    assert torch.equal(ids[1, 0], tok(["a dog"])[0])
    assert ids[2, 2, 1:11].tolist() == [tok.convert_tokens_to_ids("dog</w>")] * 10
    # the run's count can come from rows encoded elsewhere (the other embedding set, the negative prompt)
    (ids2,), c2 = T.long_ids(tok, ["a dog"], chunks=2)
    assert c2 == 2 and torch.equal(ids2[0, 1], empty)


def test_more_than_225_tokens_is_an_error_that_names_the_count(tok):
    from tweediemix_amd import text as T
    assert len(T.chunk_prompt(tok, " ".join(["cat"] * 225))) == 3
    with pytest.raises(ValueError, match="226 tokens"):
        T.chunk_prompt(tok, " ".join(["cat"] * 226))
    with pytest.raises(ValueError, match="225"):
        T.long_ids(tok, ["a cat", " ".join(["cat"] * 226)])
    with pytest.raises(ValueError, match="single word"):
        T.chunk_prompt(tok, "a " + "x" * 76)                               # one word of 76 tokens cannot be placed


def test_two_tokenizers_cut_at_the_same_words(tok, golden_dir):
    """tokenizer_2 pads with '!', so a literal '!!!' is three of its tokens and fewer of tokenizer 1's: the cut respects both"""
    from tweediemix_amd import text as T
    tok2 = T.ClipBPETokenizer.from_pretrained(os.path.join(golden_dir, "clip_tok"))
    tok2.pad_token = "!"
    prompt = " ".join(["cat !!!!!!"] * 20)
    chunks = T.chunk_prompt([tok, tok2], prompt)
    ids, c = T.long_ids([tok, tok2], [prompt])
    assert c == len(chunks) >= 2
    for t in (tok, tok2):
        assert all(len(t.tokenize(ch)) <= 75 for ch in chunks)
        assert [x for ch in chunks for x in t.tokenize(ch)] == t.tokenize(prompt)


# ------------------------------------------------------------------------------------------------ 2. token positions
def test_token_positions_long(tok):
    from tweediemix_amd import text as T
    short = "photo of a cat and a dog running, mountain background"
    assert T.token_positions_long(tok, short, "a dog") == T.phrase_token_positions(tok, short, "a dog")
    # a phrase in the second chunk: 75 fillers, then 'photo of a teddy bear' -> 'teddy bear' at offsets 4, 5 of chunk 1
    prompt = " ".join(["cat"] * 75 + ["photo", "of", "a", "teddy", "bear"])
    assert T.token_positions_long(tok, prompt, "a teddy bear") == [77 + 4, 77 + 5]
    assert T.token_positions_long(tok, prompt, "a") == [77 + 3]          # only stop-words: kept
    # a straddling phrase: 'teddy' is token 75 of chunk 0, 'bear' token 1 of chunk 1
    prompt = " ".join(["cat"] * 74 + ["teddy", "bear", "running"])
    assert T.token_positions_long(tok, prompt, "teddy bear") == [75, 77 + 1]
    with pytest.raises(ValueError, match="a horse"):
        T.token_positions_long(tok, prompt, "a horse")


# ------------------------------------------------------------------------------------------------ 3. the entry point validates
def test_xattn_token_maps_long_argument_errors():
    from tweediemix_amd import lib
    l = lib.load()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)

    def call(Q=base, K=base + 1024, maps=base + 2048, toks=(4, 100), n_tok=None, Lk=154, Sq=16, H=4, ldq=256, ldk=256):
        arr = None if toks is None else (C.c_int32 * 32)(*toks)
        n = (len(toks) if toks else 1) if n_tok is None else n_tok
        return l.tmix_xattn_token_maps_long(Q, ldq, 16 * ldq, K, ldk, 160 * ldk, maps, 2, H, Sq, Lk, 1, 1, 1, arr, n, 1, 0.125, None)

    assert call(n_tok=0) == lib.EINVAL and b"n_tok" in l.tmix_last_error_string()
    assert call(n_tok=33) == lib.EINVAL and b"n_tok" in l.tmix_last_error_string()
    assert call(Lk=241) == lib.ESHAPE and b"Lk" in l.tmix_last_error_string()
    assert call(toks=(4, 154)) == lib.EINVAL and b"token position 154" in l.tmix_last_error_string()      # position >= Lk
    assert call(toks=(4, 81), Lk=81) == lib.EINVAL
    assert call(toks=tuple(range(9)), Lk=8) == lib.EINVAL                   # 9 positions, 80 keys or fewer: the long kernel's checks
    assert call(toks=(4, 77), Lk=77) == lib.EINVAL                          # forwarded to the short form, which checks the positions
    assert call(Q=None) == lib.EINVAL and b"null" in l.tmix_last_error_string()
    assert call(K=None) == lib.EINVAL and call(maps=None) == lib.EINVAL and call(toks=None) == lib.EINVAL
    assert call(ldq=192) == lib.ESHAPE and call(Q=base + 2) == lib.EALIGN
    # the short entry point keeps its limits
    arr = (C.c_int32 * 32)(*range(9))
    assert l.tmix_xattn_token_maps(base, 256, 4096, base + 1024, 256, 20480, base + 2048, 2, 4, 16, 77, 1, 1, 1, arr, 9, 1, 0.125, None) == lib.EINVAL
    assert l.tmix_xattn_token_maps(base, 256, 4096, base + 1024, 256, 20480, base + 2048, 2, 4, 16, 81, 1, 1, 1, arr, 8, 1, 0.125, None) == lib.ESHAPE


def test_which_entry_point_a_launch_takes():
    from tweediemix_amd import ops
    assert not ops.xattn_maps_long(77, 8) and not ops.xattn_maps_long(80, 1)
    assert ops.xattn_maps_long(81, 1) and ops.xattn_maps_long(77, 9) and ops.xattn_maps_long(231, 32)


# ------------------------------------------------------------------------------------------------ 4. sampler and CLI
def test_sampler_takes_9_positions_and_refuses_33():
    from tweediemix_amd import sampler as S
    W = SimpleNamespace(device=torch.device("cpu"), kind="custom")
    cfg = S.make_config(guidance_scale=0.8, n_timesteps=10, t_cond=0.2, resampling_steps=1, jumping_steps=2, resolution_h=128, resolution_w=128)
    nine = [[4, 5, 6], [81, 82, 83], [150, 151, 152]]
    tw = S.Tweediemix(cfg, W, None, None, None, concept_num=4, attention_masks=dict(tokens=nine))
    assert tw.attention_masks["flat"] == [p for c in nine for p in c]
    S.Tweediemix(cfg, W, None, None, None, concept_num=3, attention_masks=dict(tokens=[list(range(16)), list(range(16, 32))]))
    with pytest.raises(ValueError, match="33 token positions"):
        S.Tweediemix(cfg, W, None, None, None, concept_num=3, attention_masks=dict(tokens=[list(range(16)), list(range(16, 33))]))


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_long_cpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def test_cli_parses_the_new_flags():
    fs = _cli()
    opt = fs.build_parser().parse_args([])
    assert opt.long_prompts is False and opt.synthetic_chunks == 1
    fs.check_long_prompt_args(opt)
    opt = fs.build_parser().parse_args(["--synthetic", "--long_prompts", "--synthetic_chunks", "2", "--mask_token_ids", "4,81+150"])
    assert opt.long_prompts and opt.synthetic_chunks == 2
    fs.check_long_prompt_args(opt)
    assert fs.parse_token_ids(opt.mask_token_ids) == [[4, 81], [150]]
    with pytest.raises(SystemExit, match="synthetic_chunks"):
        fs.check_long_prompt_args(fs.build_parser().parse_args(["--synthetic", "--synthetic_chunks", "2"]))
    with pytest.raises(SystemExit, match="1..3"):
        fs.check_long_prompt_args(fs.build_parser().parse_args(["--synthetic", "--long_prompts", "--synthetic_chunks", "4"]))
    e = lambda n, m: ((torch.zeros(5, n, 8), None), (torch.zeros(3, m, 8), None))
    assert fs.check_long_embeds(opt, *e(154, 154)) == 154 and fs.check_long_embeds(opt, *e(77, 77)) == 77
    with pytest.raises(SystemExit, match="77 c keys"):
        fs.check_long_embeds(opt, *e(154, 77))
    with pytest.raises(SystemExit, match="77 c keys"):
        fs.check_long_embeds(opt, *e(100, 100))


def test_cli_attention_token_lookup_uses_the_chunked_positions(tok):
    fs = _cli()
    prompt = " ".join(["cat"] * 75 + ["photo", "of", "a", "teddy", "bear", "and", "a", "dog"])
    opt = fs.build_parser().parse_args(["--long_prompts", "--prompt_orig", prompt, "--seg_concepts", "a teddy bear+a dog"])
    assert fs.attention_token_ids(opt, [tok, tok]) == [[81, 82], [85]]


def test_output_file_stem_of_a_long_prompt_fits_a_file_name():
    fs = _cli()
    assert fs.output_stem("photo of a cat and a dog+x") == "photo of a cat and a dog" and fs.output_stem("") == "sample"
    assert fs.output_stem("a" * 200) == "a" * 200                                    # what could be written before keeps its name
    long_a, long_b = "cat " * 100 + "a", "cat " * 100 + "b"
    sa, sb = fs.output_stem(long_a), fs.output_stem(long_b)
    assert sa != sb and sa.startswith("cat cat") and len(sa) == len(sb) == 160 + 9
    assert len(fs.output_stem("\u00e9" * 300).encode("utf-8")) <= 200
