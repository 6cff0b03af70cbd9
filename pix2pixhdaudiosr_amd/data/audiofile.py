"""One door for the feeder's file reads: `info` / `load` dispatch on the file's first bytes -- 'RIFF' to wavio, 'fLaC' (or an
'ID3' tag, which a FLAC stream may stand behind) to flacio -- not on the extension.  Anything else is wavio's refusal."""
from . import flacio, wavio


def kind(path):
    """'flac' or 'wav' by the first bytes of the file ('wav' for everything that is not FLAC: wavio says what is wrong with it)."""
    with open(path, "rb") as f:
        head = f.read(4)
    return "flac" if head == b"fLaC" or head[:3] == b"ID3" else "wav"


def info(path):
    return flacio.info(path) if kind(path) == "flac" else wavio.info(path)


def load(path, frame_offset=0, num_frames=-1):
    return (flacio if kind(path) == "flac" else wavio).load(path, frame_offset, num_frames)
