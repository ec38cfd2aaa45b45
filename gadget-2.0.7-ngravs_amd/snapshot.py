"""Reader for the snapshot files of Engine.write_snapshot / the reference's savepositions() (io.c), every block:

    hdr, blocks = read_blocks(path)                 # format 2: by label
    hdr, blocks = read_blocks(path, blocks_mask)    # format 1: by position, the mask says which optional blocks were written

blocks maps "POS", "VEL", "ID", "MASS", "U", "RHO", "HSML", "POT", "ACCE", "ENDT", "TSTP" to float32 arrays ([n, 3] for POS, VEL,
ACCE; int32 for ID) in the file order: type by type.  ic.read_snapshot reads the first five blocks and expands the masses."""
import struct

import numpy as np

from . import abi

HEADER_FIELDS = ("npart", "mass", "time", "redshift", "flag_sfr", "flag_feedback", "npart_total", "flag_cooling", "num_files", "box_size",
                 "omega0", "omega_lambda", "hubble_param", "flag_stellarage", "flag_metals", "npart_total_high", "flag_entropy_instead_u")


def parse_header(raw):
    """struct io_header (allvars.h), 256 bytes -> dict"""
    assert len(raw) == 256
    v = struct.unpack("<6i6d2d2i6I2i4d2i6Ii", raw[:196])
    out = dict(npart=np.array(v[0:6], dtype=np.int64), mass=np.array(v[6:12]), time=v[12], redshift=v[13], flag_sfr=v[14], flag_feedback=v[15],
               npart_total=np.array(v[16:22], dtype=np.int64), flag_cooling=v[22], num_files=v[23], box_size=v[24], omega0=v[25],
               omega_lambda=v[26], hubble_param=v[27], flag_stellarage=v[28], flag_metals=v[29],
               npart_total_high=np.array(v[30:36], dtype=np.int64), flag_entropy_instead_u=v[36])
    out["fill"] = raw[196:]
    return out


def block_count(block, npart, mass):
    """get_particles_in_block (io.c:465-523)"""
    npart = np.asarray(npart)
    if block == abi.SNAP_MASS:
        return int(npart[np.asarray(mass) == 0].sum())
    if block in abi.SNAP_GAS_BLOCKS:
        return int(npart[0])
    return int(npart.sum())


def _records(raw):
    """the Fortran-style records of the file: [length | bytes | length]"""
    recs, o = [], 0
    while o < len(raw):
        (n,) = struct.unpack_from("<i", raw, o)
        body = raw[o + 4:o + 4 + n]
        (m,) = struct.unpack_from("<i", raw, o + 4 + n)
        if m != n or len(body) != n:
            raise ValueError("record at byte %d: lengths %d and %d do not match" % (o, n, m))
        recs.append(body)
        o += n + 8
    return recs


def _typed(block, body):
    a = np.frombuffer(body, dtype=np.int32 if block == abi.SNAP_ID else np.float32)
    return a.reshape(-1, 3) if block in abi.SNAP_VECTOR_BLOCKS else a


def read_blocks(path, blocks_mask=None):
    """(header dict, {label: array}) of a snapshot file.  A format-2 file is read by its labels; a format-1 file by position: its
    records are the present blocks with elements, in the order of enum iofields, where blocks_mask (abi.snap_mask) says which of
    POT, ACCE, ENDT, TSTP are present (None: none of them)."""
    with open(path, "rb") as f:
        recs = _records(f.read())
    blocks = {}
    if len(recs[0]) == 8 and recs[0][:4] == b"HEAD":   # format 2
        hdr = parse_header(recs[1])
        for lab, body in zip(recs[2::2], recs[3::2]):
            label = lab[:4].decode()
            if struct.unpack("<i", lab[4:])[0] != len(body) + 8:
                raise ValueError("block %r: the label record does not announce the block's length" % label)
            b = abi.SNAP_LABELS.index(label)
            blocks[abi.SNAP_BLOCKS[b]] = _typed(b, body)
    else:
        hdr = parse_header(recs[0])
        mask = abi.SNAP_ALWAYS if blocks_mask is None else int(blocks_mask) | abi.SNAP_ALWAYS
        present = [b for b in range(len(abi.SNAP_BLOCKS)) if (mask >> b) & 1 and block_count(b, hdr["npart"], hdr["mass"]) > 0]
        if len(present) != len(recs) - 1:
            raise ValueError("the file has %d blocks, the mask and the header say %d" % (len(recs) - 1, len(present)))
        for b, body in zip(present, recs[1:]):
            blocks[abi.SNAP_BLOCKS[b]] = _typed(b, body)
    for name, a in blocks.items():
        b = abi.SNAP_BLOCKS.index(name)
        if len(a) != block_count(b, hdr["npart"], hdr["mass"]):
            raise ValueError("block %s has %d elements, the header says %d" % (name, len(a), block_count(b, hdr["npart"], hdr["mass"])))
    return hdr, blocks
