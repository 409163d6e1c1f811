"""h5py.File-shaped access to REAL HDF5 files through the system's HDF5 C library (ctypes on libhdf5.so).

The reference keeps everything between its stages in HDF5 (``h5py.File``): patches
(pre_processing/patch_gen_hdf5.py:66,119-120), per-slide features (compute_features_hdf5.py:110,134-135;
kmean_features.py:75-80,108) and the training reads (src/read_data.py:47-49, src/utils.py:30-33).  h5py is not
installed in this image, but the HDF5 library itself is (conda's ``libhdf5.so`` 1.10); this module binds the dozen C
entry points those call sites need, so the stores written here are ordinary HDF5 files that h5py / the reference
read unchanged, and real SEQUOIA feature files can be consumed as they are.

Subset: ``File(path, mode in {"r", "r+", "w", "a"})``, ``keys()``, ``in``, ``f[name]`` -> dataset with ``[...]``,
``shape``, ``dtype`` and ``np.asarray``; ``create_dataset(name, data=array)`` (contiguous layout, native byte order);
context manager.  Numeric dtypes: (u)int8/16/32/64, float32/64.  No filters -- none of the reference's call sites use them.

For the anndata files of the spatial analysis (spotnorm.read_h5ad) there is a little more: ``f["a/b"]`` paths, groups
(``create_group``; ``f[name]`` gives a ``Group`` for one, with the same ``keys`` / ``in`` / ``[]`` / ``create_dataset``),
``node.attrs`` with scalar strings and small integer arrays (``in``, ``[]``, ``get``, ``[] =``), and 1-D string datasets,
variable- or fixed-length, read as object arrays of ``str`` and written from a list of ``str`` (``create_dataset(name,
data=[...], string="vlen" | "fixed")``)."""
import ctypes
import ctypes.util
import glob
import os

import numpy as np

hid_t = ctypes.c_int64
hsize_t = ctypes.c_uint64

_CANDIDATES = ["/opt/conda/lib/libhdf5.so*", "/usr/lib/x86_64-linux-gnu/hdf5/serial/libhdf5.so*", "/usr/lib/x86_64-linux-gnu/libhdf5*.so*",
               "/usr/lib64/libhdf5.so*", "/usr/local/lib/libhdf5.so*"]
_lib = None
_lib_error = None

H5F_ACC_RDONLY, H5F_ACC_RDWR, H5F_ACC_TRUNC, H5F_ACC_EXCL = 0, 1, 2, 4
H5T_INTEGER, H5T_FLOAT, H5T_STRING = 0, 1, 3
H5T_CLASS_NAMES = {0: "integer", 1: "float", 2: "time", 3: "string", 4: "bitfield", 5: "opaque", 6: "compound", 7: "reference", 8: "enum",
                   9: "variable-length", 10: "array"}
H5I_GROUP, H5I_DATASET = 2, 5
H5T_VARIABLE = ctypes.c_size_t(-1).value
H5T_CSET_UTF8 = 1


def _find():
    env = os.environ.get("SEQUOIA_HDF5_LIB")
    if env:
        return [env]
    paths = []
    name = ctypes.util.find_library("hdf5")
    if name:
        paths.append(name)
    for pat in _CANDIDATES:
        paths += sorted(p for p in glob.glob(pat) if "_hl" not in p and "_cpp" not in p and "fortran" not in p)
    return paths


def library():
    """The loaded libhdf5 (ctypes.CDLL) or None when no usable HDF5 C library is present."""
    global _lib, _lib_error
    if _lib is not None or _lib_error is not None:
        return _lib
    for path in _find():
        try:
            lib = ctypes.CDLL(path)
            if lib.H5open() < 0:
                continue
            _declare(lib)
            _lib = lib
            return _lib
        except OSError as e:
            _lib_error = e
        except AttributeError as e:          # a library without the symbols we need
            _lib_error = e
    _lib_error = _lib_error or OSError("no libhdf5 found")
    return None


def available():
    return library() is not None


_ITER_CB = ctypes.CFUNCTYPE(ctypes.c_int, hid_t, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p)


def _declare(lib):
    c, vp = ctypes, ctypes.c_void_p
    sig = {
        "H5Fcreate": (hid_t, [c.c_char_p, c.c_uint, hid_t, hid_t]), "H5Fopen": (hid_t, [c.c_char_p, c.c_uint, hid_t]),
        "H5Fclose": (c.c_int, [hid_t]), "H5Fflush": (c.c_int, [hid_t, c.c_int]),
        "H5Screate_simple": (hid_t, [c.c_int, c.POINTER(hsize_t), c.POINTER(hsize_t)]), "H5Sclose": (c.c_int, [hid_t]),
        "H5Dcreate2": (hid_t, [hid_t, c.c_char_p, hid_t, hid_t, hid_t, hid_t, hid_t]),
        "H5Dopen2": (hid_t, [hid_t, c.c_char_p, hid_t]), "H5Dclose": (c.c_int, [hid_t]),
        "H5Dwrite": (c.c_int, [hid_t, hid_t, hid_t, hid_t, hid_t, vp]), "H5Dread": (c.c_int, [hid_t, hid_t, hid_t, hid_t, hid_t, vp]),
        "H5Dget_space": (hid_t, [hid_t]), "H5Dget_type": (hid_t, [hid_t]),
        "H5Sget_simple_extent_ndims": (c.c_int, [hid_t]),
        "H5Sget_simple_extent_dims": (c.c_int, [hid_t, c.POINTER(hsize_t), c.POINTER(hsize_t)]),
        "H5Tget_class": (c.c_int, [hid_t]), "H5Tget_size": (c.c_size_t, [hid_t]), "H5Tget_sign": (c.c_int, [hid_t]),
        "H5Tclose": (c.c_int, [hid_t]), "H5Lexists": (c.c_int, [hid_t, c.c_char_p, hid_t]),
        "H5Eset_auto2": (c.c_int, [hid_t, vp, vp]),
        "H5Pcreate": (hid_t, [hid_t]), "H5Pclose": (c.c_int, [hid_t]), "H5Pset_obj_track_times": (c.c_int, [hid_t, c.c_uint]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    it = getattr(lib, "H5Literate", None) or getattr(lib, "H5Literate1")
    it.restype, it.argtypes = c.c_int, [hid_t, c.c_int, c.c_int, c.POINTER(hsize_t), _ITER_CB, vp]
    lib._sq_iterate = it
    lib.H5Eset_auto2(0, None, None)          # errors come back as negative ids; no stderr stack dumps
    more = {
        "H5Gcreate2": (hid_t, [hid_t, c.c_char_p, hid_t, hid_t, hid_t]), "H5Gclose": (c.c_int, [hid_t]),
        "H5Oopen": (hid_t, [hid_t, c.c_char_p, hid_t]), "H5Oclose": (c.c_int, [hid_t]), "H5Iget_type": (c.c_int, [hid_t]),
        "H5Aexists": (c.c_int, [hid_t, c.c_char_p]), "H5Aopen": (hid_t, [hid_t, c.c_char_p, hid_t]), "H5Aclose": (c.c_int, [hid_t]),
        "H5Aget_type": (hid_t, [hid_t]), "H5Aget_space": (hid_t, [hid_t]), "H5Aread": (c.c_int, [hid_t, hid_t, vp]),
        "H5Acreate2": (hid_t, [hid_t, c.c_char_p, hid_t, hid_t, hid_t, hid_t]), "H5Awrite": (c.c_int, [hid_t, hid_t, vp]),
        "H5Screate": (hid_t, [c.c_int]), "H5Tcopy": (hid_t, [hid_t]), "H5Tset_size": (c.c_int, [hid_t, c.c_size_t]),
        "H5Tset_cset": (c.c_int, [hid_t, c.c_int]), "H5Tis_variable_str": (c.c_int, [hid_t]),
        "H5Dvlen_reclaim": (c.c_int, [hid_t, hid_t, hid_t, vp]),
    }
    try:                                     # groups, attributes and strings: the feature stores never need them
        for name, (res, args) in more.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._sq_objects = True
    except AttributeError:
        lib._sq_objects = False


_NATIVE = {"u1": "UINT8", "i1": "INT8", "u2": "UINT16", "i2": "INT16", "u4": "UINT32", "i4": "INT32", "u8": "UINT64",
           "i8": "INT64", "f4": "FLOAT", "f8": "DOUBLE"}


def _native_type(dtype):
    dt = np.dtype(dtype)
    key = dt.kind + str(dt.itemsize)
    if key not in _NATIVE:
        raise TypeError(f"h5lite: dtype {dt} is not supported (numeric (u)int8..64 / float32 / float64 only)")
    return hid_t.in_dll(library(), f"H5T_NATIVE_{_NATIVE[key]}_g").value


def _need_objects(lib):
    if not getattr(lib, "_sq_objects", False):
        raise OSError("h5lite: this libhdf5 lacks the group / attribute / string entry points")


def _string_type(lib, size):
    """A UTF-8 C string type of ``size`` bytes (H5T_VARIABLE: variable length); the caller closes it."""
    tid = lib.H5Tcopy(hid_t.in_dll(lib, "H5T_C_S1_g").value)
    if tid < 0 or lib.H5Tset_size(tid, size) < 0 or lib.H5Tset_cset(tid, H5T_CSET_UTF8) < 0:
        raise OSError("h5lite: making a string type failed")
    return tid


def _read_strings(lib, file_type, shape, read, name):
    """The strings of a dataset or attribute of string type ``file_type`` and shape () or (n,) as an object array of str
    (a str for shape ()).  ``read(memory type, buffer)`` is the H5Dread / H5Aread call."""
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    out = np.empty(n, dtype=object)
    if lib.H5Tis_variable_str(file_type) > 0:
        mem = _string_type(lib, H5T_VARIABLE)
        buf = (ctypes.c_void_p * max(n, 1))()
        dims = (hsize_t * 1)(n)
        sid = lib.H5Screate_simple(1, dims, None)
        try:
            if n and read(mem, ctypes.cast(buf, ctypes.c_void_p)) < 0:
                raise OSError(f"h5lite: reading the strings of '{name}' failed")
            for i in range(n):
                out[i] = ctypes.string_at(buf[i]).decode("utf-8") if buf[i] else ""
            if n:
                lib.H5Dvlen_reclaim(mem, sid, 0, ctypes.cast(buf, ctypes.c_void_p))       # the library allocated every string
        finally:
            lib.H5Sclose(sid)
            lib.H5Tclose(mem)
    else:
        size = int(lib.H5Tget_size(file_type))
        mem = lib.H5Tcopy(file_type)                         # the file's own padding and character set: no conversion
        raw = np.zeros(max(n, 1), dtype=f"S{size}")
        try:
            if n and read(mem, raw.ctypes.data_as(ctypes.c_void_p)) < 0:
                raise OSError(f"h5lite: reading the strings of '{name}' failed")
        finally:
            lib.H5Tclose(mem)
        for i in range(n):
            out[i] = bytes(raw[i]).rstrip(b" ").decode("utf-8")      # numpy has dropped the trailing NULs; space padding goes too
    return out.reshape(shape) if shape else out[0]


class Attributes:
    """``node.attrs``: scalar strings and integer arrays of a group or dataset.  ``in``, ``[]``, ``get``, ``[] =``."""

    def __init__(self, file, path):
        _need_objects(file._lib)
        self._file, self._path = file, path

    def _open(self):
        oid = self._file._lib.H5Oopen(self._file._fid, self._path.encode(), 0)
        if oid < 0:
            raise KeyError(f"Unable to open object (object '{self._path}' doesn't exist)")
        return oid

    def __contains__(self, name):
        lib, oid = self._file._lib, self._open()
        try:
            return lib.H5Aexists(oid, name.encode()) > 0
        finally:
            lib.H5Oclose(oid)

    def get(self, name, default=None):
        return self[name] if name in self else default

    def __getitem__(self, name):
        lib, oid = self._file._lib, self._open()
        aid = -1
        try:
            if lib.H5Aexists(oid, name.encode()) <= 0:
                raise KeyError(f"Can't open attribute (can't locate attribute: '{name}')")
            aid = lib.H5Aopen(oid, name.encode(), 0)
            if aid < 0:
                raise OSError(f"h5lite: opening attribute '{name}' of '{self._path}' failed")
            sid, tid = lib.H5Aget_space(aid), lib.H5Aget_type(aid)
            try:
                nd = lib.H5Sget_simple_extent_ndims(sid)
                dims = (hsize_t * max(nd, 1))()
                if nd > 0:
                    lib.H5Sget_simple_extent_dims(sid, dims, None)
                shape = tuple(int(dims[i]) for i in range(max(nd, 0)))
                cls, size, sign = lib.H5Tget_class(tid), lib.H5Tget_size(tid), lib.H5Tget_sign(tid)
                if cls == H5T_STRING and nd <= 1:
                    return _read_strings(lib, tid, shape, lambda mem, buf: lib.H5Aread(aid, mem, buf), name)
                if cls in (H5T_INTEGER, H5T_FLOAT):
                    dt = np.dtype(f"f{size}") if cls == H5T_FLOAT else np.dtype(("i" if sign == 1 else "u") + str(size))
                    buf = np.empty(shape, dtype=dt)
                    if buf.size and lib.H5Aread(aid, _native_type(dt), buf.ctypes.data_as(ctypes.c_void_p)) < 0:
                        raise OSError(f"h5lite: reading attribute '{name}' of '{self._path}' failed")
                    return buf if shape else buf[()]
                raise TypeError(f"h5lite: attribute '{name}' of '{self._path}' has HDF5 type class {cls} ({H5T_CLASS_NAMES.get(cls, '?')}); "
                                f"only strings and numbers are supported")
            finally:
                lib.H5Tclose(tid)
                lib.H5Sclose(sid)
        finally:
            if aid >= 0:
                lib.H5Aclose(aid)
            lib.H5Oclose(oid)

    def __setitem__(self, name, value):
        if self._file.mode == "r":
            raise OSError("h5lite: file opened read-only")
        lib, oid = self._file._lib, self._open()
        tid, sid, aid, own_type = -1, -1, -1, False
        try:
            if lib.H5Aexists(oid, name.encode()) > 0:
                raise ValueError(f"Unable to create attribute (name already exists): {name}")
            if isinstance(value, str):                       # a scalar variable-length UTF-8 string, as anndata writes them
                tid, own_type = _string_type(lib, H5T_VARIABLE), True
                sid = lib.H5Screate(0)                       # H5S_SCALAR
                text = ctypes.c_char_p(value.encode("utf-8"))
                data = ctypes.cast(ctypes.pointer(text), ctypes.c_void_p)
            else:
                arr = np.ascontiguousarray(np.asarray(value))
                if arr.dtype.kind not in "iu" or arr.ndim > 1:
                    raise TypeError(f"h5lite: attribute '{name}': a str or a 1-D integer array is expected, got {arr.dtype} {arr.shape}")
                tid = _native_type(arr.dtype)
                dims = (hsize_t * max(arr.ndim, 1))(*arr.shape)
                sid = lib.H5Screate_simple(arr.ndim, dims, None) if arr.ndim else lib.H5Screate(0)
                data = arr.ctypes.data_as(ctypes.c_void_p)
            aid = lib.H5Acreate2(oid, name.encode(), tid, sid, 0, 0)
            if aid < 0 or lib.H5Awrite(aid, tid, data) < 0:
                raise OSError(f"h5lite: writing attribute '{name}' of '{self._path}' failed")
        finally:
            if aid >= 0:
                lib.H5Aclose(aid)
            if sid >= 0:
                lib.H5Sclose(sid)
            if own_type:
                lib.H5Tclose(tid)
            lib.H5Oclose(oid)


class Dataset:
    """A dataset handle that behaves like the slice of h5py the call sites use: ``ds[:]``, ``ds[...]``, ``ds[i:j]``,
    ``np.asarray(ds)``, ``.shape``, ``.dtype``.  The whole dataset is read on first access (features are a few MB)."""

    def __init__(self, lib, fid, name, file=None):
        self._lib, self.name, self._file = lib, name, file
        did = lib.H5Dopen2(fid, name.encode(), 0)
        if did < 0:
            raise KeyError(f"Unable to open object (object '{name}' doesn't exist)")
        try:
            sid = lib.H5Dget_space(did)
            nd = lib.H5Sget_simple_extent_ndims(sid)
            dims = (hsize_t * max(nd, 1))()
            if nd > 0:
                lib.H5Sget_simple_extent_dims(sid, dims, None)
            lib.H5Sclose(sid)
            tid = lib.H5Dget_type(did)
            cls, size, sign = lib.H5Tget_class(tid), lib.H5Tget_size(tid), lib.H5Tget_sign(tid)
            if cls == H5T_STRING and getattr(lib, "_sq_objects", False) and nd <= 1:
                self.shape = tuple(int(dims[i]) for i in range(nd))
                self.dtype = np.dtype(object)
                try:
                    self._data = _read_strings(lib, tid, self.shape, lambda mem, buf: lib.H5Dread(did, mem, 0, 0, 0, buf), name)
                finally:
                    lib.H5Tclose(tid)
                return
            lib.H5Tclose(tid)
            if cls == H5T_FLOAT:
                dt = np.dtype(f"f{size}")
            elif cls == H5T_INTEGER:
                dt = np.dtype(("i" if sign == 1 else "u") + str(size))
            else:
                raise TypeError(f"h5lite: dataset '{name}' has HDF5 type class {cls} ({H5T_CLASS_NAMES.get(cls, '?')}); only integer / float "
                                f"datasets and 1-D string datasets are supported")
            self.shape = tuple(int(dims[i]) for i in range(nd))
            self.dtype = dt
            buf = np.empty(self.shape, dtype=dt)
            if buf.size and lib.H5Dread(did, _native_type(dt), 0, 0, 0, buf.ctypes.data_as(ctypes.c_void_p)) < 0:
                raise OSError(f"h5lite: reading dataset '{name}' failed")
            self._data = buf
        finally:
            lib.H5Dclose(did)

    def __getitem__(self, key):
        return self._data[key]

    def __array__(self, dtype=None, copy=None):
        return self._data if dtype is None else self._data.astype(dtype)

    def __len__(self):
        return self.shape[0]

    @property
    def attrs(self):
        return Attributes(self._file, self.name)


class Group:
    """A group below the root: what ``f[name]`` gives for one.  Names are relative to it; every call goes through the
    file with the full path."""

    def __init__(self, file, path):
        self._file, self.name = file, path.strip("/")

    def _full(self, name):
        return self.name + "/" + name.strip("/")

    def keys(self):
        return self._file._keys(self.name)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def __contains__(self, name):
        return self._full(name) in self._file

    def __getitem__(self, name):
        return self._file[self._full(name)]

    def kind(self, name):
        return self._file.kind(self._full(name))

    def create_group(self, name):
        return self._file.create_group(self._full(name))

    def create_dataset(self, name, data=None, shape=None, dtype=None, string=None):
        return self._file.create_dataset(self._full(name), data=data, shape=shape, dtype=dtype, string=string)

    @property
    def attrs(self):
        return Attributes(self._file, self.name)


class File:
    def __init__(self, path, mode="r"):
        lib = library()
        if lib is None:
            raise OSError(f"h5lite: no HDF5 C library available ({_lib_error})")
        self._lib, self.filename, self.mode = lib, path, mode
        p = os.fsencode(path)
        if mode == "r":
            fid = lib.H5Fopen(p, H5F_ACC_RDONLY, 0)
        elif mode == "r+":
            fid = lib.H5Fopen(p, H5F_ACC_RDWR, 0)
        elif mode == "w":
            fid = lib.H5Fcreate(p, H5F_ACC_TRUNC, 0, 0)
        elif mode == "a":
            fid = lib.H5Fopen(p, H5F_ACC_RDWR, 0) if os.path.exists(path) else lib.H5Fcreate(p, H5F_ACC_EXCL, 0, 0)
        else:
            raise ValueError(f"h5lite: mode {mode!r}")
        if fid < 0:
            raise OSError(f"Unable to open file (unable to open file: name = '{path}', mode = '{mode}')")
        self._fid = fid

    # -- reading -------------------------------------------------------------------------------------------------
    def keys(self):
        return self._keys("")

    def _keys(self, path):
        """The link names of the root (``""``) or of the group ``path``."""
        names = []

        @_ITER_CB
        def cb(g, name, info, data):
            names.append(name.decode())
            return 0
        idx = hsize_t(0)
        loc = self._fid
        if path:
            _need_objects(self._lib)
            loc = self._lib.H5Oopen(self._fid, path.encode(), 0)
            if loc < 0:
                raise KeyError(f"Unable to open object (object '{path}' doesn't exist)")
        try:
            if self._lib._sq_iterate(loc, 0, 0, ctypes.byref(idx), cb, None) < 0:        # H5_INDEX_NAME, H5_ITER_INC
                raise OSError("h5lite: link iteration failed")
        finally:
            if path:
                self._lib.H5Oclose(loc)
        return names

    def kind(self, name):
        """"group" or "dataset" (anything else: "other") for the object at ``name``; KeyError if there is none."""
        _need_objects(self._lib)
        if name not in self:
            raise KeyError(f"Unable to open object (object '{name}' doesn't exist)")
        oid = self._lib.H5Oopen(self._fid, name.encode(), 0)
        if oid < 0:
            raise KeyError(f"Unable to open object (object '{name}' doesn't exist)")
        try:
            return {H5I_GROUP: "group", H5I_DATASET: "dataset"}.get(self._lib.H5Iget_type(oid), "other")
        finally:
            self._lib.H5Oclose(oid)

    def type_class(self, name):
        """The HDF5 type class of the dataset ``name`` as a word ("integer", "float", "string", "compound", ...)."""
        did = self._lib.H5Dopen2(self._fid, name.encode(), 0)
        if did < 0:
            raise KeyError(f"Unable to open object (object '{name}' doesn't exist)")
        try:
            tid = self._lib.H5Dget_type(did)
            cls = self._lib.H5Tget_class(tid)
            self._lib.H5Tclose(tid)
            return H5T_CLASS_NAMES.get(cls, str(cls))
        finally:
            self._lib.H5Dclose(did)

    @property
    def attrs(self):
        return Attributes(self, "/")

    def create_group(self, name):
        _need_objects(self._lib)
        if self.mode == "r":
            raise OSError("h5lite: file opened read-only")
        if name in self:
            raise ValueError(f"Unable to create group (name already exists): {name}")
        gid = self._lib.H5Gcreate2(self._fid, name.encode(), 0, 0, 0)
        if gid < 0:
            raise OSError(f"h5lite: creating group '{name}' failed")
        self._lib.H5Gclose(gid)
        return Group(self, name)

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def __contains__(self, name):
        return self._lib.H5Lexists(self._fid, name.encode(), 0) > 0

    def __getitem__(self, name):
        if name not in self:
            raise KeyError(f"Unable to open object (object '{name}' doesn't exist)")
        if getattr(self._lib, "_sq_objects", False) and self.kind(name) == "group":
            return Group(self, name)
        return Dataset(self._lib, self._fid, name, file=self)

    # -- writing -------------------------------------------------------------------------------------------------
    def _create_strings(self, name, values, string):
        """A 1-D UTF-8 string dataset: string = "vlen" (variable length) or "fixed" (the longest value's bytes + 1)."""
        lib = self._lib
        _need_objects(lib)
        enc = [str(v).encode("utf-8") for v in values]
        if string == "vlen":
            tid = _string_type(lib, H5T_VARIABLE)
            buf = (ctypes.c_char_p * max(len(enc), 1))(*enc)
            data = ctypes.cast(buf, ctypes.c_void_p)
        elif string == "fixed":
            size = max([len(e) for e in enc] + [0]) + 1      # a null-terminated type keeps its last byte for the terminator
            tid = _string_type(lib, size)
            buf = np.array(enc, dtype=f"S{size}") if enc else np.zeros(1, dtype=f"S{size}")
            data = buf.ctypes.data_as(ctypes.c_void_p)
        else:
            raise ValueError(f"h5lite: string = {string!r}, must be 'vlen' or 'fixed'")
        dims = (hsize_t * 1)(len(enc))
        sid = lib.H5Screate_simple(1, dims, None)
        did = lib.H5Dcreate2(self._fid, name.encode(), tid, sid, 0, 0, 0)
        try:
            if did < 0:
                raise OSError(f"h5lite: creating dataset '{name}' failed")
            if enc and lib.H5Dwrite(did, tid, 0, 0, 0, data) < 0:
                raise OSError(f"h5lite: writing dataset '{name}' failed")
        finally:
            if did >= 0:
                lib.H5Dclose(did)
            lib.H5Sclose(sid)
            lib.H5Tclose(tid)
        return Dataset(lib, self._fid, name, file=self)

    def create_dataset(self, name, data=None, shape=None, dtype=None, string=None):
        if self.mode == "r":
            raise OSError("h5lite: file opened read-only")
        if string is not None:
            if name in self:
                raise ValueError(f"Unable to create dataset (name already exists): {name}")
            return self._create_strings(name, data, string)
        if data is None:
            data = np.zeros(shape, dtype=dtype or np.float32)
        arr = np.ascontiguousarray(np.asarray(data))
        if dtype is not None:
            arr = np.ascontiguousarray(arr.astype(dtype))
        if arr.dtype.byteorder == ">":
            arr = arr.astype(arr.dtype.newbyteorder("="))
        lib = self._lib
        if name in self:
            raise ValueError(f"Unable to create dataset (name already exists): {name}")
        tid = _native_type(arr.dtype)
        dims = (hsize_t * max(arr.ndim, 1))(*arr.shape)
        sid = lib.H5Screate_simple(arr.ndim, dims, None)
        # h5py's default (track_times=False): no creation / modification stamps in the object header, so a file's bytes are a
        # function of its contents -- the files of a sharded run can be compared with the one-rank run's byte for byte
        try:
            dcpl = lib.H5Pcreate(hid_t.in_dll(lib, "H5P_CLS_DATASET_CREATE_ID_g").value)
        except ValueError:                       # a build that does not export the property-list class id: default creation properties
            dcpl = -1
        if dcpl >= 0:
            lib.H5Pset_obj_track_times(dcpl, 0)
        did = lib.H5Dcreate2(self._fid, name.encode(), tid, sid, 0, max(dcpl, 0), 0)
        try:
            if did < 0:
                raise OSError(f"h5lite: creating dataset '{name}' failed")
            if arr.size and lib.H5Dwrite(did, tid, 0, 0, 0, arr.ctypes.data_as(ctypes.c_void_p)) < 0:
                raise OSError(f"h5lite: writing dataset '{name}' failed")
        finally:
            if did >= 0:
                lib.H5Dclose(did)
            if dcpl >= 0:
                lib.H5Pclose(dcpl)
            lib.H5Sclose(sid)
        return Dataset(lib, self._fid, name, file=self)

    def flush(self):
        self._lib.H5Fflush(self._fid, 1)

    def close(self):
        if self._fid is not None:
            self._lib.H5Fclose(self._fid)
            self._fid = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            if getattr(self, "_fid", None) is not None:
                self.close()
        except Exception:
            pass
