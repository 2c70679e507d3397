"""The build's source list against the source directory (no GPU): build.py compiles exactly the .hip / .cpp files that lie
in csrc -- a file nobody lists would silently not be built, a listed name without a file is a misspelling -- and the
translation units on the FFT core of csrc/fft_core.h get the default flags: the fused onset and pitch kernels are compiled
with floating-point contraction on (onset_terms.h / pitch_terms.h switch it off for themselves), unlike kernels_onset.hip
and kernels_pitch.hip."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT_CORE_UNITS = ["kernels_stft_block.hip", "kernels_stft_feat.hip", "kernels_resynth_batch.hip", "kernels_onset_fused.hip",
                  "kernels_pitch_fused.hip"]


def _build():
    spec = importlib.util.spec_from_file_location("fluhip_build_src", os.path.join(ROOT, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sources_are_exactly_the_files_of_csrc():
    b = _build()
    on_disk = sorted(f for f in os.listdir(b.CSRC) if f.endswith((".hip", ".cpp")))
    assert len(b.SOURCES) == len(set(b.SOURCES)), sorted(s for s in set(b.SOURCES) if b.SOURCES.count(s) > 1)
    orphans = sorted(set(on_disk) - set(b.SOURCES))      # in csrc, not built
    phantoms = sorted(set(b.SOURCES) - set(on_disk))     # listed, not there
    assert not orphans and not phantoms, (orphans, phantoms)


def test_the_fft_core_units_take_the_default_flags():
    b = _build()
    assert set(FFT_CORE_UNITS) <= set(b.SOURCES)
    assert not set(FFT_CORE_UNITS) & set(b.EXTRA_FLAGS), sorted(set(FFT_CORE_UNITS) & set(b.EXTRA_FLAGS))
