"""One door for the feeder's file reads: `info` / `load` dispatch on the file's first bytes -- 'RIFF' to wavio, 'fLaC' (or an
'ID3' tag, which a FLAC stream may stand behind) to flacio, 'FORM' (AIFF / AIFF-C), '.snd' (AU) and 'NIST' (SPHERE) to containers --
not on the extension.  Anything else is wavio's refusal.  So a TIMIT `.WAV` file, which is a SPHERE file, loads."""
from . import containers, flacio, wavio


def kind(path):
    """'flac', 'aiff', 'au', 'sphere' or 'wav' by the first bytes of the file ('wav' for everything that is none of the others:
    wavio says what is wrong with it)."""
    with open(path, "rb") as f:
        head = f.read(4)
    if head == b"fLaC" or head[:3] == b"ID3":
        return "flac"
    return containers.kind_of(head) or "wav"


def _reader(path):
    k = kind(path)
    return flacio if k == "flac" else wavio if k == "wav" else containers


def info(path):
    return _reader(path).info(path)


def load(path, frame_offset=0, num_frames=-1):
    return _reader(path).load(path, frame_offset, num_frames)
