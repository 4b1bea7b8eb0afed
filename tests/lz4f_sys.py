"""TEST INFRASTRUCTURE ONLY: the frame API (lz4frame.h) of the image's system
liblz4 through ctypes, to pin the LZ4 frame oracle (tests/lz4f_ref.py).  Never
loaded by the product."""
import ctypes
import ctypes.util

_sz, _vp, _u = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint


class FrameInfo(ctypes.Structure):
    _fields_ = [("blockSizeID", ctypes.c_int), ("blockMode", ctypes.c_int), ("contentChecksumFlag", ctypes.c_int),
                ("frameType", ctypes.c_int), ("contentSize", ctypes.c_ulonglong), ("dictID", _u),
                ("blockChecksumFlag", ctypes.c_int)]


class Preferences(ctypes.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", ctypes.c_int), ("autoFlush", _u),
                ("favorDecSpeed", _u), ("reserved", _u * 3)]


LINKED, INDEPENDENT = 0, 1
VERSION = 100


def load():
    for name in ("liblz4.so.1", ctypes.util.find_library("lz4")):
        if not name:
            continue
        try:
            L = ctypes.CDLL(name)
        except OSError:
            continue
        if not hasattr(L, "LZ4F_compressFrame"):
            continue
        P = ctypes.POINTER(Preferences)
        L.LZ4F_isError.argtypes = [_sz]
        L.LZ4F_compressFrameBound.argtypes = [_sz, P]
        L.LZ4F_compressFrameBound.restype = _sz
        L.LZ4F_compressFrame.argtypes = [_vp, _sz, ctypes.c_char_p, _sz, P]
        L.LZ4F_compressFrame.restype = _sz
        L.LZ4F_compressBound.argtypes = [_sz, P]
        L.LZ4F_compressBound.restype = _sz
        L.LZ4F_createCompressionContext.argtypes = [ctypes.POINTER(_vp), _u]
        L.LZ4F_createCompressionContext.restype = _sz
        L.LZ4F_freeCompressionContext.argtypes = [_vp]
        L.LZ4F_compressBegin.argtypes = [_vp, _vp, _sz, P]
        L.LZ4F_compressBegin.restype = _sz
        L.LZ4F_compressUpdate.argtypes = [_vp, _vp, _sz, ctypes.c_char_p, _sz, _vp]
        L.LZ4F_compressUpdate.restype = _sz
        L.LZ4F_flush.argtypes = [_vp, _vp, _sz, _vp]
        L.LZ4F_flush.restype = _sz
        L.LZ4F_compressEnd.argtypes = [_vp, _vp, _sz, _vp]
        L.LZ4F_compressEnd.restype = _sz
        L.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(_vp), _u]
        L.LZ4F_createDecompressionContext.restype = _sz
        L.LZ4F_freeDecompressionContext.argtypes = [_vp]
        L.LZ4F_decompress.argtypes = [_vp, _vp, ctypes.POINTER(_sz), ctypes.c_char_p, ctypes.POINTER(_sz), _vp]
        L.LZ4F_decompress.restype = _sz
        L.LZ4_versionNumber.restype = ctypes.c_int
        return L
    return None


class SysLz4F:
    def __init__(self, L):
        self.L = L
        self.version = L.LZ4_versionNumber()

    @staticmethod
    def prefs(bid=4, mode=INDEPENDENT, checksum=False, bsum=False, size=0):
        p = Preferences()
        p.frameInfo.blockSizeID = bid
        p.frameInfo.blockMode = mode
        p.frameInfo.contentChecksumFlag = int(checksum)
        p.frameInfo.blockChecksumFlag = int(bsum)
        p.frameInfo.contentSize = size
        return p

    def bound(self, n: int, bid: int = 4, checksum: bool = True) -> int:
        p = self.prefs(bid, checksum=checksum, size=n)
        return self.L.LZ4F_compressFrameBound(n, ctypes.byref(p))

    def compress_frame(self, x: bytes, bid=4, checksum=False, mode=INDEPENDENT, bsum=False, size=True) -> bytes:
        """LZ4F_compressFrame, level 0; size: write contentSize = len(x)."""
        p = self.prefs(bid, mode, checksum, bsum, len(x) if size else 0)
        cap = self.L.LZ4F_compressFrameBound(len(x), ctypes.byref(p))
        out = ctypes.create_string_buffer(cap)
        n = self.L.LZ4F_compressFrame(out, cap, x, len(x), ctypes.byref(p))
        assert not self.L.LZ4F_isError(n)
        return out.raw[:n]

    def compress_pieces(self, pieces, bid=4, mode=INDEPENDENT, checksum=False, bsum=False, size=None) -> bytes:
        """LZ4F_compressBegin / Update / flush per piece / End: a block ends
        wherever a piece does, so non-final blocks may be short."""
        L = self.L
        p = self.prefs(bid, mode, checksum, bsum, size or 0)
        ctx = _vp()
        assert not L.LZ4F_isError(L.LZ4F_createCompressionContext(ctypes.byref(ctx), VERSION))
        cap = 64 + sum(L.LZ4F_compressBound(len(x), ctypes.byref(p)) + 16 for x in pieces) + \
            L.LZ4F_compressBound(0, ctypes.byref(p))
        buf = ctypes.create_string_buffer(cap)
        base = ctypes.addressof(buf)
        pos = 0

        def step(n):
            nonlocal pos
            assert not L.LZ4F_isError(n), n
            pos += n
        step(L.LZ4F_compressBegin(ctx, base, cap, ctypes.byref(p)))
        for x in pieces:
            step(L.LZ4F_compressUpdate(ctx, base + pos, cap - pos, x, len(x), None))
            step(L.LZ4F_flush(ctx, base + pos, cap - pos, None))
        step(L.LZ4F_compressEnd(ctx, base + pos, cap - pos, None))
        L.LZ4F_freeCompressionContext(ctx)
        return buf.raw[:pos]

    def decompress(self, f: bytes, cap: int):
        """(accepted, bytes or None): accepted when LZ4F_decompress ends the
        frame having consumed exactly the body and produced at most cap bytes."""
        L = self.L
        ctx = _vp()
        assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(ctypes.byref(ctx), VERSION))
        out = ctypes.create_string_buffer(cap + 1)
        base = ctypes.addressof(out)
        ip = op = 0
        ok = False
        try:
            while True:
                dn, sn = _sz(cap + 1 - op), _sz(len(f) - ip)
                r = L.LZ4F_decompress(ctx, base + op, ctypes.byref(dn), f[ip:], ctypes.byref(sn), None)
                if L.LZ4F_isError(r):
                    break
                ip += sn.value
                op += dn.value
                if r == 0:
                    ok = ip == len(f) and op <= cap
                    break
                if op > cap or (sn.value == 0 and dn.value == 0):
                    break
        finally:
            L.LZ4F_freeDecompressionContext(ctx)
        return ok, (out.raw[:op] if ok else None)
