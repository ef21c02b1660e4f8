"""Resource checks of the built device code (CPU only: the kernel descriptors of
libspai.so's gfx950 code object, scripts/kernel_regs.py).  The hot kernels must use
no scratch memory: a register array indexed by a loop that stayed rolled lands on
the scratch stack and silently costs the forward several times its time (round 6:
one build of the C4 forward spilled its B/A rings there at S = 4).  The C4 forward's
register footprint must also leave a tree-kernel wave room beside it on the SIMD
(<= 464 of 512), which is what lets one search chain's select run
under the other chain's forward."""
import os
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "scripts"))
LIB = os.path.join(REPO, "self-play-ai_amd", "libspai.so")

HOT = ["k_forwardILb0E", "k_forwardILb1E", "k_selectILb0E", "k_expand_selectILb0E", "k_advance", "k_chess_forward",
       "k_cleaf", "k_cexpand", "k_legal4", "k_apply4", "k_encodeILb1E"]


@pytest.fixture(scope="module")
def descriptors():
    if not os.path.exists(LIB):
        pytest.skip("libspai.so not built")
    import kernel_regs
    return kernel_regs.kernels(LIB)


@pytest.mark.parametrize("kernel", HOT)
def test_hot_kernels_use_no_scratch(descriptors, kernel):
    hits = {n: f for n, f in descriptors.items() if kernel in n}
    assert hits, kernel
    for n, f in hits.items():
        assert int(f["private_segment_fixed_size"]) == 0, (n, f["private_segment_fixed_size"])


def test_c4_forward_register_budget(descriptors):
    for n, f in descriptors.items():
        if "k_forwardILb0E" in n:
            assert int(f["vgpr_count"]) <= 464, (n, f["vgpr_count"])
            assert int(f["vgpr_spill_count"]) == 0, (n, f["vgpr_spill_count"])


def test_no_compile_time_variants_in_kernels():
    """The kernels carry no experiment behind a preprocessor switch: a measured and
    rejected variant lives in git history and DESIGN.md, not in the product source.
    Only the diagnostic (phase-stamp) family may be a conditional on an SPAI_ macro."""
    import glob
    import re
    cond = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")
    files = sorted(glob.glob(os.path.join(REPO, "self-play-ai_amd", "csrc", "*.hip")))
    assert files
    bad = []
    for path in files:
        for no, line in enumerate(open(path), 1):
            m = cond.match(line)
            for macro in re.findall(r"\bSPAI_\w+", m.group(1)) if m else []:
                if not macro.startswith("SPAI_DIAG"):
                    bad.append("%s:%d: %s" % (os.path.basename(path), no, macro))
    assert not bad, bad


def test_c4_learner_builds_only_the_kernels_it_launches(descriptors):
    """The Connect4 train step has one path, and learner.hip instantiates exactly what
    that path can launch: k_conv_mfma<4,4> (the stem), <32,1> and <64,1> (launch_conv's
    three-way dispatch on the padded input channels), k_wgrad_mfma<4> and <64>, and one
    k_heads_loss.  An instantiation that no launch reaches is dead weight in the code
    object (at one time two thirds of the learner's .text)."""
    import re

    def tails(kernel):   # the mangled template arguments (and parameters) after the kernel's name
        return sorted(m.group(1) for m in (re.search(r"\d+%s(\w*)$" % kernel, n) for n in descriptors) if m)

    conv, wgrad, heads = tails("k_conv_mfma"), tails("k_wgrad_mfma"), tails("k_heads_loss")
    assert [t.split("EE")[0] for t in conv] == ["ILi32ELi1", "ILi4ELi4", "ILi64ELi1"], conv
    assert [t.split("EE")[0] for t in wgrad] == ["ILi4", "ILi64"], wgrad
    assert len(heads) == 1, heads


def test_every_environment_knob_is_documented():
    """every "SPAI_..." string literal of the library's sources (a getenv name) has its
    row in INTEGRATION.md's "Environment knobs" section"""
    import glob
    import re
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    section = doc.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    files = sorted(glob.glob(os.path.join(REPO, "self-play-ai_amd", "csrc", "*")))
    names = {m for path in files if os.path.isfile(path) for m in re.findall(r'"(SPAI_\w+)"', open(path).read())}
    assert "SPAI_TRACE_MOVES" in names   # the scan finds the literals
    missing = sorted(n for n in names if not re.search(r"\b%s\b" % n, section))
    assert not missing, missing
