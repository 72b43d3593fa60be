"""Does the formant correction move the formants: the whole vowel table of profiles/r25_formant.txt, the rows without a threshold included.
CPU, the fp64 reference only (tests/formant_reference.py); tests/test_formant_cpu.py asserts the +4 and +7 rows at 120 and 150 Hz.

    python scripts/formant_vowels.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F0S = (120.0, 150.0, 200.0)
SEMITONES = (4, 7, -5, -12)


def main():
    from tests import formant_reference as R
    from tests.test_formant_cpu import H, N, Q, VOWEL_FORMANTS, vowel_distances
    from tortoise_tts_amd import formant as fmt
    print("# source-filter vowel, formants %s Hz, Q = %d, clamp 24 dB; distances in dB rms (DESIGN.md 5.32)" % (VOWEL_FORMANTS, Q))
    print("#   F0 Hz  semitones  corrected  shifted  floor  corrected / shifted")
    for f0 in F0S:
        for s in SEMITONES:
            c, sh, fl = vowel_distances(f0, s, lambda p: R.Tables(fmt.tables(Q, [p]), N, H))
            print("#   %5.0f  %+9d  %9.2f  %7.2f  %5.2f   %.2f" % (f0, s, c, sh, fl, c / sh))


if __name__ == "__main__":
    main()
