"""Peak-file front door: pick the reader / writer by file extension (the role of the reference's
falcon/ms_io/ms_io.py:11-66).  MGF, mzML and mzXML are read (the extension test is case-insensitive); only MGF is written.
The XML readers also hand their binary arrays, still encoded, to the device decoder (`read_chunks`); MGF text is parsed on the
device as a whole (`device_reader`), with `mgf_io.get_spectra` as the reader of record; the structure of mzML is scanned on the
device (`device_chunk_reader`), with `mzml_io.read_chunks` as the reader of record."""
import os

from . import mgf_io, mzml_io, mzxml_io

_READERS = {".mgf": mgf_io.get_spectra, ".mzml": mzml_io.get_spectra, ".mzxml": mzxml_io.get_spectra}
_CHUNK_READERS = {".mzml": mzml_io.read_chunks, ".mzxml": mzxml_io.read_chunks}
_DEVICE_READERS = {".mgf": mgf_io.read_chunks}
_DEVICE_CHUNK_READERS = {".mzml": mzml_io.read_chunks_device}
_WRITERS = {".mgf": mgf_io.write_spectra}


def _extension(path: str) -> str:
    return os.path.splitext(path.lower())[1]


def get_spectra(filename: str):
    """Iterate over the spectra of a peak file as plain dicts (see mgf_io.get_spectra)."""
    if not os.path.isfile(filename):
        raise ValueError(f"Non-existing peak file {filename}")
    reader = _READERS.get(_extension(filename))
    if reader is None:
        raise ValueError(f'Unknown spectrum file type with extension "{_extension(filename)}"')
    yield from reader(filename)


def chunk_reader(filename: str):
    """the `read_chunks(filename, max_bytes)` of an mzML / mzXML file (spectra + still-encoded arrays), None for other types"""
    return _CHUNK_READERS.get(_extension(filename))


def device_reader(filename: str):
    """the `read_chunks(filename, ctx, max_bytes)` of an MGF file, whose text is parsed on the device; None for other types"""
    return _DEVICE_READERS.get(_extension(filename))


def device_chunk_reader(filename: str):
    """the `read_chunks_device(filename, ctx, max_bytes)` of an mzML file, whose structure is scanned on the device and whose chunks
    are `chunk_reader`'s with the payload left on the device; None for other types (mzXML stays on its host reader)"""
    return _DEVICE_CHUNK_READERS.get(_extension(filename))


def write_spectra(filename: str, spectra) -> None:
    """Write spectra (dicts) to a peak file; like the reference (ms_io.py:58-66) only MGF can be written."""
    writer = _WRITERS.get(_extension(filename))
    if writer is None:
        raise ValueError("Unsupported output file format (only MGF can be written)")
    writer(filename, spectra)


def write_representatives(filename: str, ctx, *columns, **options) -> str:
    """Write cluster representatives held as columns (`mgf_io.write_representatives`: peaks CSR, rows, precursor m/z, retention
    time, charge, cluster id, titles) to a peak file, formatted on the device; only MGF can be written."""
    if _extension(filename) != ".mgf":
        raise ValueError("Unsupported output file format (only MGF can be written)")
    return mgf_io.write_representatives(filename, ctx, *columns, **options)
