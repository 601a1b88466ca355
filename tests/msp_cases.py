"""Texts and references for the MSP library reader (`falcon_amd/ms_io/msp_io.py`, `csrc/mspparse.h`, `csrc/mspparse.hip`).

No real MSP file is at hand offline: the three texts below are hand-written in the three common styles (NIST: several `mz int;`
per line and quoted annotations; MoNA: one peak per line and `Comments:`; a matchms export: upper-case keys and tab-separated
peaks), with the values the grammar of `msp_io`'s docstring gives them spelled out beside them.  Then designed entries for every
rule, a plain restatement of the grammar over bytes in the C ABI's terms (`expected_parse`, `expected_headers`), and a writer of
one synthetic library in both formats."""
import re

import numpy as np

WS = b" \t\r\n"

NIST = """Name: Caffeine
MW: 194
Formula: C8H10N4O2
CAS#: 58-08-2;  NIST#: 1234
DB#: 101
Comments: "NIST style; with a semicolon"
PrecursorMZ: 195.0877
Precursor_type: [M+H]+
Ion_mode: P
Charge: 1
Num Peaks: 7
42.0338 5.5; 69.0447 12.1; 83.0604 4;
110.0713 60.25 "C5H8N3 1/2; p"
138.0662 999 "parent-C2H3NO";
163.0 1; 195.0877 100 "precursor"

Name: Theobromine; 3,7-dimethylxanthine
MW: 180
DB#: 102
PrecursorMZ: 181.072 100
Precursor_type: [M+H]+
Num Peaks: 3
67.0291 20; 110.0349 45;
181.0720 999 "p";
"""
NIST_WANT = [
    dict(identifier="101", name="Caffeine", precursor_mz=195.0877, precursor_charge=1, adduct="[M+H]+", ionmode="P", smiles="", inchikey="",
         mz=[42.0338, 69.0447, 83.0604, 110.0713, 138.0662, 163.0, 195.0877], intensity=[5.5, 12.1, 4, 60.25, 999, 1, 100]),
    dict(identifier="102", name="Theobromine; 3,7-dimethylxanthine", precursor_mz=181.072, precursor_charge=0, adduct="[M+H]+", ionmode="",
         smiles="", inchikey="", mz=[67.0291, 110.0349, 181.072], intensity=[20, 45, 999]),
]

MONA = """Name: Quercetin
Synon: $:00in-source
DB#: MoNA000123
InChIKey: REFJWTPEDVJJIY-UHFFFAOYSA-N
Precursor_type: [M-H]-
Spectrum_type: MS2
PrecursorMZ: 301.0354
Instrument_type: LC-ESI-QTOF
Ion_mode: N
Comments: "SMILES=O=C1C(O)=C(OC2=CC(O)=CC(O)=C12)C3=CC=C(O)C(O)=C3" "computed mass=302.0427"
Num Peaks: 4
107.0139 10.5
151.0037 100
178.9986 45.25
301.0354 80

Name: Kaempferol
DB#: MoNA000124
InChIKey: IYRMWMYZSQPJKC-UHFFFAOYSA-N
SMILES: C1=CC(=CC=C1C2=C(C(=O)C3=C(C=C(C=C3O2)O)O)O)O
Precursor_type: [M+H]+
PrecursorMZ: 287.055
Ion_mode: P
Num Peaks: 2
153.0182 100
287.0550 35.5
"""
MONA_WANT = [
    dict(identifier="MoNA000123", name="Quercetin", precursor_mz=301.0354, precursor_charge=0, adduct="[M-H]-", ionmode="N", smiles="",
         inchikey="REFJWTPEDVJJIY-UHFFFAOYSA-N", mz=[107.0139, 151.0037, 178.9986, 301.0354], intensity=[10.5, 100, 45.25, 80]),
    dict(identifier="MoNA000124", name="Kaempferol", precursor_mz=287.055, precursor_charge=0, adduct="[M+H]+", ionmode="P",
         smiles="C1=CC(=CC=C1C2=C(C(=O)C3=C(C=C(C=C3O2)O)O)O)O", inchikey="IYRMWMYZSQPJKC-UHFFFAOYSA-N", mz=[153.0182, 287.055],
         intensity=[100, 35.5]),
]

MATCHMS = """NAME: Glucose
PRECURSOR_MZ: 203.0526
CHARGE: 1
IONMODE: positive
ADDUCT: [M+Na]+
SMILES: OCC1OC(O)C(O)C(O)C1O
INCHIKEY: WQZGKKKJIJFFOK-UHFFFAOYSA-N
SPECTRUMID: CCMSLIB00000001
NUM PEAKS: 3
85.0284\t0.12
203.0526\t1.0
143.0315\t0.5

NAME: Fructose
PRECURSOR_MZ: 179.0561
CHARGE: -1
IONMODE: negative
ADDUCT: [M-H]-
SPECTRUMID: CCMSLIB00000002
NUM PEAKS: 2
59.0139\t0.3
89.0244\t1.0
"""
MATCHMS_WANT = [
    dict(identifier="CCMSLIB00000001", name="Glucose", precursor_mz=203.0526, precursor_charge=1, adduct="[M+Na]+", ionmode="positive",
         smiles="OCC1OC(O)C(O)C(O)C1O", inchikey="WQZGKKKJIJFFOK-UHFFFAOYSA-N", mz=[85.0284, 203.0526, 143.0315], intensity=[0.12, 1.0, 0.5]),
    # ("-1": `_parse_charge` takes the sign behind the digits only and int("-1") stands; the value is the host reader's)
    dict(identifier="CCMSLIB00000002", name="Fructose", precursor_mz=179.0561, precursor_charge=-1, adduct="[M-H]-", ionmode="negative",
         smiles="", inchikey="", mz=[59.0139, 89.0244], intensity=[0.3, 1.0]),
]
STYLES = {"nist": (NIST, NIST_WANT), "mona": (MONA, MONA_WANT), "matchms": (MATCHMS, MATCHMS_WANT)}

PEAKS = ("100.5 1.0", "200.25 3.5", "150.125 2.0")


def entry(name, *header, pm="PrecursorMZ: 500.5", num="auto", peaks=PEAKS, blank=True):
    """one entry as text: `Name:`, `pm` (None: no precursor line), the header lines, `Num Peaks:` (`num`; "auto": the number of
    peak lines; None: no such line), the peak lines"""
    lines = [f"Name: {name}"] + ([pm] if pm else []) + list(header)
    if num is not None:
        lines.append(f"Num Peaks: {len(peaks) if num == 'auto' else num}")
    return "\n".join(lines + list(peaks) + ([""] if blank else [])) + "\n"


E = entry
# (entry text, what the reader makes of it: None = skipped, else the fields that the case is about)
DESIGNED = [
    (E("precursormz first", "Precursor_MZ: 2.5", "PEPMASS: 3.5", pm="PrecursorMZ: 1.5"), dict(precursor_mz=1.5)),
    (E("precursor_mz second", "PEPMASS: 3.5", pm="PRECURSOR_MZ: 2.5"), dict(precursor_mz=2.5)),
    (E("pepmass third", pm="PepMass: 3.5 1000"), dict(precursor_mz=3.5)),
    (E("an empty alias falls through", "Precursor_MZ: 2.5", pm="PrecursorMZ:"), dict(precursor_mz=2.5)),
    (E("last line wins", "PrecursorMZ: 700.25", "Charge: 1", "Charge: 2-", "SMILES: C", "smiles : CC=O "), dict(precursor_mz=700.25, precursor_charge=-2, smiles="CC=O")),
    (E("spectrumid", "Accession: A1", "DB#: D1", "SpectrumID: S1"), dict(identifier="S1")),
    (E("db#", "Accession: A1", "DB#: D1", "SpectrumID:"), dict(identifier="D1")),
    (E("accession", "Accession: A1"), dict(identifier="A1")),
    (E("no identifier"), dict(identifier="designed.msp:9")),
    (E("precursor_type before adduct", "Adduct: second", "Precursor_type: first", "IonMode: second", "Ion_mode: first"), dict(adduct="first", ionmode="first")),
    (E("adduct and ionmode", "Adduct: [M+H]+", "IONMODE: Positive", "InChIKey: KEY-1"), dict(adduct="[M+H]+", ionmode="Positive", inchikey="KEY-1")),
    (E("no precursor", pm=None), None),
    (E("unparsable precursor", pm="PrecursorMZ: abc"), None),
    (E("infinite precursor", pm="PrecursorMZ: inf"), None),
    (E("nan precursor", pm="PrecursorMZ: nan"), None),
    (E("zero precursor", pm="PrecursorMZ: 0"), None),
    (E("negative precursor", pm="PrecursorMZ: -5"), None),
    (E("no num peaks", num=None), None),
    (E("num peaks int() rejects", num="3 4"), None),
    (E("fewer peaks than declared", num="4"), None),
    (E("more peaks than declared", num="2"), None),
    (E("a malformed m/z", peaks=("100.5 1", "abc 2", "3 4")), None),
    (E("a malformed intensity", peaks=("100.5 1", "2 x", "3 4")), None),
    (E("num peaks int() takes", num="+03", peaks=("5 1; 4 2;", "3 \"note; 9 9\"")), dict(mz=[5.0, 4.0, 3.0], intensity=[1.0, 2.0, 0.0])),
    (E("float() forms", num="3", peaks=("1_0 1e2; .5 5.", "\t+7\t\t8\tfurther tokens 9")), dict(mz=[10.0, 0.5, 7.0], intensity=[100.0, 5.0, 8.0])),
    (E("no peaks", num="0", peaks=()), dict(mz=[], intensity=[])),
    (E("blank lines inside", "", "Charge: 3", "", num="2", peaks=("1 2", "", "  ", "3 4")), dict(precursor_charge=3, mz=[1.0, 3.0], intensity=[2.0, 4.0])),
    (E("a line without a colon is ignored", "just words", "Charge 5"), dict(precursor_charge=0)),
    (E("charge forms", "Charge: 2+ and 3+"), dict(precursor_charge=2)),
    (E("a charge _parse_charge rejects", "Charge: positive"), dict(precursor_charge=0)),
    (E("an empty charge", "Charge:"), dict(precursor_charge=0)),
    (E("a header-shaped line behind num peaks is peak text", peaks=("100.5 1", "Comment: x", "3 4")), None),
    (E("a second num peaks line is peak text", peaks=("1 2", "Num Peaks: 3", "3 4")), None),
    (E("with: colons ", "NAMES: not the name"), dict(name="with: colons")),
]


# ---- the grammar over bytes, in the C ABI's terms ---------------------------------------------------------------------------------
_DOUBLE = re.compile(rb"[+-]?(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")


def fast_double(tok: bytes):
    """mgfparse.h's number fast form: float(tok) when the token is decided on the device, None when it is the host's"""
    m = _DOUBLE.fullmatch(tok)
    if not m:
        return None
    whole, frac = (m.group(1) or b""), (m.group(2) or b"") if m.group(1) is not None else m.group(3)
    digits = (whole + frac).lstrip(b"0")
    if len(digits) > 19:
        return None
    if not digits:
        return float(tok)
    q = min(max(int(m.group(4) or b"0"), -10 ** 6), 10 ** 6) - len(frac)
    return float(tok) if -27 <= q <= 27 else None


def fast_charge(tok: bytes):
    m = re.fullmatch(rb"([0-9]{1,9})([+-]?)", tok)
    return None if not m else (-int(m.group(1)) if m.group(2) == b"-" else int(m.group(1)))


def fast_count(tok: bytes):
    return int(tok) if re.fullmatch(rb"[0-9]{1,9}", tok) else None


def split_line(line: bytes):
    """a stripped line -> (lower-case key or None when there is no ':', offset of the value in the line, stripped value)"""
    if b":" not in line:
        return None, len(line), b""
    k, v = line.split(b":", 1)
    lead = len(v) - len(v.lstrip(WS))
    return k.strip(WS).lower(), len(k) + 1 + lead, v.strip(WS)


def segments(line: bytes):
    """the peak segments of a line: what stands before the first '"', split at ';', non-empty after stripping"""
    return [s.strip(WS) for s in line.split(b'"', 1)[0].split(b";") if s.strip(WS)]


def _lines(text: bytes):
    pos = 0
    for raw in text.split(b"\n"):
        yield pos, raw
        pos += len(raw) + 1


def expected_parse(text: bytes):
    """fal_msp_index + fal_msp_parse over `text` as include/falcon_hip.h states them -> dict: n, indptr, span, status, and for
    the entries the device decides (status 0) precursor_mz, charge, has_charge and the peaks sorted by m/z (stable)"""
    rows = [(pos, raw, raw.strip(WS)) for pos, raw in _lines(text)]
    begins = [i for i, (_, _, s) in enumerate(rows) if s and split_line(s)[0] == b"name"]
    out = dict(n=len(begins), indptr=[0], span=[], status=[], precursor_mz=[], charge=[], has_charge=[], mz=[], intensity=[])
    for e, b in enumerate(begins):
        end = begins[e + 1] if e + 1 < len(begins) else len(rows)
        np_line = next((i for i in range(b + 1, end) if rows[i][2] and split_line(rows[i][2])[0] == b"num peaks"), None)
        host = np_line is None
        params = {}
        for i in range(b, end if np_line is None else np_line + 1):
            s = rows[i][2]
            host |= len(s) > 4096
            key, _, value = split_line(s) if s else (None, 0, b"")
            if key is not None:
                params[key] = value
        peaks = []
        if np_line is not None:
            for i in range(np_line + 1, end):
                s = rows[i][2]
                host |= len(s) > 4096
                for seg in segments(s):
                    tok = seg.split()
                    m, v = fast_double(tok[0]), (fast_double(tok[1]) if len(tok) > 1 else 0.0)
                    host |= m is None or v is None
                    peaks.append((m, v))
        alias = next((k for k in (b"precursormz", b"precursor_mz", b"pepmass") if k in params), None)
        pm = fast_double(params[alias].split()[0]) if alias and params[alias] else None
        charge = fast_charge(params[b"charge"]) if b"charge" in params else 0
        count = fast_count(params.get(b"num peaks", b""))
        host |= pm is None or charge is None or count is None or count != len(peaks)
        out["indptr"].append(out["indptr"][-1] + len(peaks))
        out["span"].append((rows[b][0], min(rows[end][0], len(text)) if end < len(rows) else len(text)))
        out["status"].append(int(host))
        order = sorted(range(len(peaks)), key=lambda j: peaks[j][0]) if not host else []
        out["precursor_mz"].append(None if host else pm)
        out["charge"].append(None if host else charge)
        out["has_charge"].append(None if host else int(b"charge" in params))
        out["mz"].append(None if host else np.array([peaks[j][0] for j in order], np.float64))
        out["intensity"].append(None if host else np.array([peaks[j][1] for j in order], np.float64).astype(np.float32))
    return out


def expected_headers(text: bytes, keys: dict, PRESENT=1, HOST=2, INT=1):
    """fal_msp_headers over `text` -> span i64[n, k, 2], value i64[n, k], state i32[n, k]: per entry and key the last line of that
    key among the lines from the Name: line to the first Num Peaks line"""
    names = [k.encode("ascii") for k in keys]
    kinds = list(keys.values())
    rows = [(pos, raw, raw.strip(WS)) for pos, raw in _lines(text)]
    begins = [i for i, (_, _, s) in enumerate(rows) if s and split_line(s)[0] == b"name"]
    n = len(begins)
    span, value, state = np.zeros((n, len(names), 2), np.int64), np.zeros((n, len(names)), np.int64), np.zeros((n, len(names)), np.int32)
    for e, b in enumerate(begins):
        end = begins[e + 1] if e + 1 < n else len(rows)
        for i in range(b, end):
            pos, raw, s = rows[i]
            key, off, v = split_line(s) if s else (None, 0, b"")
            if key in names:
                j = names.index(key)
                lo = pos + (len(raw) - len(raw.lstrip(WS))) + off
                span[e, j] = lo, lo + len(v)
                state[e, j], value[e, j] = PRESENT, 0
                if len(s) > 4096:
                    state[e, j] = HOST
                elif kinds[j] == INT and v:
                    if re.fullmatch(rb"[+-]?[0-9]{1,18}", v):
                        value[e, j] = int(v)
                    else:
                        state[e, j] = HOST
            if key == b"num peaks":
                break
    return span, value, state


# ---- one synthetic library in both formats ----------------------------------------------------------------------------------------
def both_formats(entries):
    """entries -- dicts of `pm` (text), `charge` (int, 0: no line), `name`, `sid`, `adduct`, `smiles`, `inchikey`, `ionmode` and
    `peaks` ("mz intensity" texts) -- -> (MGF text, MSP text): the same strings and the same float texts in both; the MSP entries
    alternate between one peak per line and four per line with `;`"""
    mgf, msp = [], []
    for i, e in enumerate(entries):
        ch, peaks = ([f"{e['charge']}+"] if e["charge"] else []), list(e["peaks"])
        mgf += ["BEGIN IONS", f"PEPMASS={e['pm']}"] + [f"CHARGE={c}" for c in ch] + [f"NAME={e['name']}", f"SPECTRUMID={e['sid']}",
                f"ADDUCT={e['adduct']}", f"SMILES={e['smiles']}", f"INCHIKEY={e['inchikey']}", f"IONMODE={e['ionmode']}"] + peaks + ["END IONS", ""]
        msp += [f"Name: {e['name']}", f"SpectrumID: {e['sid']}", f"PrecursorMZ: {e['pm']}"] + [f"Charge: {c}" for c in ch] + [
                f"Precursor_type: {e['adduct']}", f"SMILES: {e['smiles']}", f"InChIKey: {e['inchikey']}", f"Ion_mode: {e['ionmode']}",
                f"Num Peaks: {len(peaks)}"]
        msp += ["; ".join(peaks[j:j + 4]) + (";" if i % 4 == 1 else "") for j in range(0, len(peaks), 4)] if i % 2 else peaks
        msp.append("")
    return "\n".join(mgf) + "\n", "\n".join(msp) + "\n"


def random_entries(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        mz, k = np.sort(rng.uniform(120.0, 1400.0, int(rng.integers(6, 40)))), int(rng.integers(0, 3))
        out.append(dict(pm=f"{float(rng.uniform(300, 1400)):.4f}", charge=k, name=f"compound {i}, form {i % 7}", sid=f"LIB{i:08d}",
                        adduct=["[M+H]+", "[M+Na]+", "[M-H]-"][i % 3], smiles="C" * (i % 9 + 1) + "=O", inchikey=f"KEY{i:08d}-UHFFFAOYSA-N",
                        ionmode=["Positive", "Negative"][i % 2], peaks=[f"{float(a):.4f} {float(b):.2f}" for a, b in zip(mz, rng.uniform(1.0, 1e5, len(mz)))]))
    return out
