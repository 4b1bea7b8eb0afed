# Top-level build (no cmake): HIP codec library for gfx950, host C++ layer,
# synthetic-data generator, and the test-only oracle.  `make -j8`.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
PKG      := flare-cpp_amd
LIB      := $(PKG)/lib
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall
CSRC     := $(PKG)/csrc/capi.hip $(PKG)/csrc/snappy_decode.hip $(PKG)/csrc/snappy_decode_v3.hip $(PKG)/csrc/snappy_decode_v4.hip $(PKG)/csrc/snappy_decode_partial.hip \
            $(PKG)/csrc/snappy_encode.hip $(PKG)/csrc/snappy_encode_v3.hip $(PKG)/csrc/snappy_encode_wave.hip $(PKG)/csrc/gather.hip $(PKG)/csrc/pack.hip $(PKG)/csrc/lz4.hip $(PKG)/csrc/lz4_decode2.hip $(PKG)/csrc/lz4_encode_wave.hip $(PKG)/csrc/lz4_frame_encode.hip $(PKG)/csrc/lz4_frame_decode.hip $(PKG)/csrc/inflate.hip $(PKG)/csrc/inflate_units.hip $(PKG)/csrc/deflate.hip $(PKG)/csrc/deflate_level.hip
CHDRS    := $(wildcard $(PKG)/csrc/*.h) include/flare_snappy_gpu.h include/flare_lz4_gpu.h include/flare_deflate_gpu.h include/flare_deflate_compress_gpu.h include/flare_deflate_level_gpu.h include/flare_deflate_index_gpu.h
OBJDIR   := build/obj

all: gpu host datagen oracle cpptests hostbench echobench

gpu: $(LIB)/libflare_snappy_gpu.so

$(OBJDIR)/%.o: $(PKG)/csrc/%.hip $(CHDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB)/libflare_snappy_gpu.so: $(patsubst $(PKG)/csrc/%.hip,$(OBJDIR)/%.o,$(CSRC))
	@mkdir -p $(LIB)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# Host C++ layer (cord_buf, CompressHandler registry, GPU-backed snappy
# handler + flat API): host-only code built with g++ against the HIP runtime.
HOSTCXX   := g++ -std=c++17 -O2 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
HOST_SRC  := $(wildcard $(PKG)/host/*.cc)
HOST_HDRS := $(wildcard $(PKG)/host/*.h) include/flare_snappy_gpu.h $(PKG)/csrc/lz4_frame_format.h $(PKG)/csrc/inflate_format.h $(PKG)/csrc/deflate_format.h $(PKG)/csrc/gzip_index.h
host: $(LIB)/libflare_rpc_snappy.so

$(LIB)/libflare_rpc_snappy.so: $(HOST_SRC) $(HOST_HDRS) $(LIB)/libflare_snappy_gpu.so
	@mkdir -p $(LIB)
	$(HOSTCXX) -shared -o $@ $(HOST_SRC) -L$(LIB) -lflare_snappy_gpu -L/opt/rocm/lib -lamdhip64 \
	  -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib -pthread

# C++ tests mirroring test/rpc/rpc_snappy_compress_test.cc and the baidu_std /
# rpc_dump framing (run by pytest)
cpptests: build/test_rpc_snappy_compress build/test_baidu_std build/test_pack_output build/test_path_report build/test_lz4_frame_handler build/test_gzip_handler build/test_gzip_options build/test_gzip_unit_index

# the LZ4 frame CompressHandler (policy::Lz4FrameCompress / Lz4FrameDecompress), host only
build/test_lz4_frame_handler: tests/cpp/test_lz4_frame_handler.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# the gzip / zlib CompressHandlers (policy::GzipCompress and its kin), host only
build/test_gzip_handler: tests/cpp/test_gzip_handler.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# GzipCompress with GzipCompressOptions (format and compression level), host only
build/test_gzip_options: tests/cpp/test_gzip_options.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# GzipCompressOptions::unit_index (gzip bodies that carry their units' lengths), host only
build/test_gzip_unit_index: tests/cpp/test_gzip_unit_index.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# the runtime's device-path counters (fsh_device_path_stats)
build/test_path_report: tests/cpp/test_path_report.cc $(HOST_HDRS) include/flare_snappy_host.h $(LIB)/libflare_rpc_snappy.so $(LIB)/libflare_datagen.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu -lflare_datagen \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# the handler's packed compress path (outputs packed on the device before the D2H)
build/test_pack_output: tests/cpp/test_pack_output.cc $(HOST_HDRS) include/flare_snappy_host.h $(LIB)/libflare_rpc_snappy.so $(LIB)/libflare_datagen.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu -lflare_datagen \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

build/test_baidu_std: tests/cpp/test_baidu_std.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

build/test_rpc_snappy_compress: tests/cpp/test_rpc_snappy_compress.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# Config 1: echo over loopback (baidu_std framing, SNAPPY request/response)
echobench: build/echo_bench
build/echo_bench: tools/echo_bench.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so $(LIB)/libflare_datagen.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu -lflare_datagen \
	  -L/opt/rocm/lib -lamdhip64 -ldl -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

# End-to-end rate of the host drop-in path (cord_buf in, cord_buf out)
hostbench: build/host_bench build/pack_latency
# p50 latency of small compress batches with the packed output path on / off
build/pack_latency: tools/pack_latency.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so $(LIB)/libflare_datagen.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu -lflare_datagen \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread
build/host_bench: tools/host_bench.cc $(HOST_HDRS) $(LIB)/libflare_rpc_snappy.so $(LIB)/libflare_datagen.so
	@mkdir -p build
	$(HOSTCXX) -o $@ $< -I$(PKG)/host -L$(LIB) -lflare_rpc_snappy -lflare_snappy_gpu -lflare_datagen \
	  -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,$(abspath $(LIB)) -Wl,-rpath,'$$ORIGIN/../$(LIB)' \
	  -Wl,-rpath,/opt/rocm/lib -pthread

datagen: $(LIB)/libflare_datagen.so

$(LIB)/libflare_datagen.so: $(PKG)/tools/datagen.c
	@mkdir -p $(LIB)
	gcc -std=c11 -O2 -fPIC -shared -pthread -o $@ $< -lm

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf build $(LIB)/*.so
	$(MAKE) -C oracle clean

.PHONY: all gpu host cpptests hostbench echobench datagen oracle clean

# Diagnostic build: exec_kernel phase stamps (s_memtime), never loaded by the
# product path.  python tools/stamps.py runs it.
stamps: $(LIB)/libflare_snappy_gpu_stamps.so
$(LIB)/libflare_snappy_gpu_stamps.so: $(CSRC) $(CHDRS)
	@mkdir -p $(LIB) build/stamps
	for f in $(CSRC); do $(HIPCC) $(HIPFLAGS) -DFSG_STAMPS -c $$f -o build/stamps/$$(basename $$f .hip).o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ build/stamps/*.o
.PHONY: stamps

# Diagnostic builds for tools/deflate_bench.py: the deflate unit kernel cut
# after phase 1 (parse) and after phase 2 (code build); never loaded by the
# product path.
deflate_phases: $(LIB)/libflare_snappy_gpu_deflate_p1.so $(LIB)/libflare_snappy_gpu_deflate_p2.so
$(LIB)/libflare_snappy_gpu_deflate_p%.so: $(PKG)/csrc/deflate.hip $(PKG)/csrc/deflate_level.hip $(CHDRS) $(LIB)/libflare_snappy_gpu.so
	@mkdir -p $(LIB) build/deflate_p$*
	$(HIPCC) $(HIPFLAGS) -DFSG_DEFLATE_PHASES=$* -c $(PKG)/csrc/deflate.hip -o build/deflate_p$*/deflate.o
	$(HIPCC) $(HIPFLAGS) -DFSG_DEFLATE_PHASES=$* -c $(PKG)/csrc/deflate_level.hip -o build/deflate_p$*/deflate_level.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ build/deflate_p$*/deflate.o build/deflate_p$*/deflate_level.o $(filter-out $(OBJDIR)/deflate.o $(OBJDIR)/deflate_level.o,$(patsubst $(PKG)/csrc/%.hip,$(OBJDIR)/%.o,$(CSRC)))
.PHONY: deflate_phases
