"""The --vocoder-fp16 switch of the offline driver and the S2ST agent (off by default) and its C-ABI entry in the loader's table."""
import argparse
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_offline_driver_flag():
    from streamspeech_amd import offline
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "out"]
    assert offline.build_parser().parse_args(base).vocoder_fp16 is False
    assert offline.build_parser().parse_args(base + ["--vocoder-fp16"]).vocoder_fp16 is True
    # fairseq's --fp16 halves the S2UT model, not the vocoder: not taken here
    assert not any("--fp16" in a.option_strings for a in offline.build_parser()._actions)


def test_agent_flag():
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    p = argparse.ArgumentParser()
    StreamSpeechS2STAgent.add_args(p)
    base = ["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0"]
    assert p.parse_args(base).vocoder_fp16 is False
    assert p.parse_args(base + ["--vocoder-fp16"]).vocoder_fp16 is True


def test_set_f16_in_header_and_loader_table():
    from streamspeech_amd import lib as L
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    for name, args in (("ss_vocoder_set_f16", 2), ("ss_op_conv_f16", 18), ("ss_prof_enable_hi", 1)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == args, name
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", header)


def test_engine_switch_is_inherited():
    import inspect
    from streamspeech_amd.engine import HipVocoder
    assert "set_fp16" in HipVocoder.__dict__
    assert "set_fp16(True)" in inspect.getsource(HipVocoder.new_context)
