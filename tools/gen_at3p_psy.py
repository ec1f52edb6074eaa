#!/usr/bin/env python3
"""Write the two integer tables of MASKING-WEIGHTED WORD LENGTHS (include/at3phip.h, M2) to atracdenc_amd/csrc/at3p_psy.inc. The
committed integers are the definition; this file says where they came from. Everything is in steps of one index of G, the squared
scale table: a factor 2^(2/3) of energy, 10 log10(2^(2/3)) = 2.007 dB.

  AT3P_PSY_SPREAD[q'][q]  how many steps under the energy of masker unit q' the threshold it casts on unit q lies: z(f) = 13 atan(0.00076 f)
      + 3.5 atan((f / 7500)^2) Bark at each unit's centre frequency (line k is centred at (k + 0.5) * 22050 / 2048 Hz), dz = z(q) - z(q'),
      12 + 10 dz dB for dz >= 0 and 12 + 27 (-dz) dB below, rounded to steps (halves up); above 63 steps: 255, no masking.
  AT3P_PSY_ATH[q]         the threshold in quiet as an index i of lambda_i: the curve the ATRAC3 path holds (the table kAthMilliBel of
      atracdenc_amd/csrc/at3_tables.cpp, read from that file, as ath_db interpolates it, - 100 - 0.015 f^2 with f in kHz: dB relative to a
      full-scale sine) at every line's centre, the minimum over the unit's lines; energy = E_FS * 10^(dB / 10); index =
      floor(1.5 log2(energy)) + 63, not below 0.
  E_FS  the spectrum energy per frame (the sum of the squares of the 2048 lines the writer is handed) of a full-scale 1 kHz sine.
      Measured once with the oracle's filter bank and transform (tests/at3p_writer_lib.py, specs_of_pcm, on
      sin(2 pi 1000 t / 44100) at amplitude 1.0, mono, 208 frames): after a start-up of 8 frames the energy swings between 0.241 and
      0.389 with the sine's phase in the frame, and its mean over frames 8..207 is 0.3147.

With --check nothing is written: the tables are formed again and compared with the committed file; the exit status is 1 if they differ."""
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "atracdenc_amd", "csrc", "at3p_psy.inc")
ATH_SRC = os.path.join(ROOT, "atracdenc_amd", "csrc", "at3_tables.cpp")
E_FS = 0.3147
STEP_DB = 10.0 * math.log10(2.0 ** (2.0 / 3.0))
SMR_DB, SLOPE_UP, SLOPE_DOWN = 12.0, 10.0, 27.0
QU_START = [0, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408,
            1536, 1664, 1792, 1920, 2048]
LINE_HZ = 22050.0 / 2048.0


def ath_millibel():
    t = open(ATH_SRC).read()
    t = t[t.index("kAthMilliBel[]"):]
    return [int(x) for x in re.findall(r"-?\d+", t[t.index("{") + 1:t.index("}")])]


def ath_db(freq, tab):
    freq = min(max(freq, 10.0), 29853.0)
    fl = 40.0 * math.log10(0.1 * freq)
    idx = int(fl)
    return 0.01 * (tab[idx] * (1 + idx - fl) + tab[idx + 1] * (fl - idx))


def bark(f):
    return 13.0 * math.atan(0.00076 * f) + 3.5 * math.atan((f / 7500.0) ** 2)


def tables():
    tab = ath_millibel()
    ath = []
    for q in range(32):
        db = min(ath_db((k + 0.5) * LINE_HZ, tab) - 100.0 - 0.015 * ((k + 0.5) * LINE_HZ * 1e-3) ** 2 for k in range(QU_START[q], QU_START[q + 1]))
        ath.append(max(0, math.floor(1.5 * math.log2(E_FS * 10.0 ** (db / 10.0))) + 63))
    z = [bark(0.5 * (QU_START[q] + QU_START[q + 1]) * LINE_HZ) for q in range(32)]
    spread = []
    for m in range(32):
        row = []
        for q in range(32):
            dz = z[q] - z[m]
            db = SMR_DB + (SLOPE_UP * dz if dz >= 0 else SLOPE_DOWN * -dz)
            s = int(math.floor(db / STEP_DB + 0.5))
            row.append(s if s <= 63 else 255)
        spread.append(row)
    return spread, ath


def text():
    spread, ath = tables()
    out = ["// Written by tools/gen_at3p_psy.py - the two integer tables of MASKING-WEIGHTED WORD LENGTHS (include/at3phip.h, M2). Data only.",
           "// AT3P_PSY_SPREAD[q'][q]: steps of G by which masker unit q' casts its threshold on unit q; 255: none.",
           "static const uint8_t AT3P_PSY_SPREAD[32][32] = {"]
    for row in spread:
        out.append("    {" + ", ".join(f"{v:3d}" for v in row) + "},")
    out += ["};", "// AT3P_PSY_ATH[q]: the threshold in quiet of unit q as an index of lambda.", "static const uint8_t AT3P_PSY_ATH[32] = {",
            "    " + ", ".join(str(v) for v in ath[:16]) + ",", "    " + ", ".join(str(v) for v in ath[16:]) + "};", ""]
    return "\n".join(out)


def main():
    t = text()
    if "--check" in sys.argv[1:]:
        if not os.path.exists(OUT) or open(OUT).read() != t:
            print(f"{OUT} differs from what this generator writes", file=sys.stderr)
            return 1
        return 0
    with open(OUT, "w") as f:
        f.write(t)
    return 0


if __name__ == "__main__":
    sys.exit(main())
