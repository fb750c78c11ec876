# Top-level build: libntt_mi355x.so (HIP, gfx950), the CPU oracle and the CPU
# emulation of the kernel templates used by the tests.
#
#   make            product library only
#   make all-test   + oracle, reference oracle (if /root/reference exists), emulator
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
PKG      = optimized-number-theoretic-transform-implementations_amd
CSRC     = $(PKG)/csrc
LIB      = $(PKG)/libntt_mi355x.so
HIPFLAGS ?= -O3 --offload-arch=$(ARCH) -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden \
            -Wall -Wextra -Wno-unused-parameter -Iinclude -Iinclude/internal -I$(CSRC) $(EXTRA_HIPFLAGS)
# (longest translation units first: `make -j` starts them in this order, and the four FP64 block-kernel units take two minutes each)
OBJS     = $(CSRC)/inst_f64k0.o $(CSRC)/inst_f64k1.o $(CSRC)/inst_f64k18.o $(CSRC)/inst_f64w.o \
           $(CSRC)/inst_dm_u64x_k0.o $(CSRC)/inst_dm_u64x_k1.o $(CSRC)/inst_dm_u64x_k3.o $(CSRC)/inst_u64x_k0.o $(CSRC)/inst_u64x_k1.o $(CSRC)/inst_u64x_k3.o \
           $(CSRC)/inst_u64.o $(CSRC)/inst_u64r4.o \
           $(CSRC)/inst_dot_f64k0.o $(CSRC)/inst_dot_f64k1.o $(CSRC)/inst_dot_f64k18.o $(CSRC)/inst_dot_f64w.o $(CSRC)/inst_dot_u64.o \
           $(CSRC)/inst_mul_f64k0.o $(CSRC)/inst_mul_f64k1.o $(CSRC)/inst_mul_f64k18.o $(CSRC)/inst_mul_f64w.o $(CSRC)/inst_mul_u64.o \
           $(CSRC)/inst_team_f64k0.o $(CSRC)/inst_team_f64k1.o $(CSRC)/inst_team_f64k18.o $(CSRC)/inst_team_f64w.o \
           $(CSRC)/rescale_f64k0.o $(CSRC)/rescale_f64k1.o $(CSRC)/rescale_f64k18.o $(CSRC)/rescale_f64w.o $(CSRC)/rescale_coef.o \
           $(CSRC)/lift_f64k0.o $(CSRC)/lift_f64k1.o $(CSRC)/lift_f64k18.o $(CSRC)/lift_f64w.o $(CSRC)/lift.o \
           $(CSRC)/sample_f64k0.o $(CSRC)/sample_f64k1.o $(CSRC)/sample_f64k18.o $(CSRC)/sample_f64w.o $(CSRC)/sample.o \
           $(CSRC)/slots_f64k0.o $(CSRC)/slots_f64k1.o $(CSRC)/slots_f64k18.o $(CSRC)/slots_f64w.o $(CSRC)/slots.o \
           $(CSRC)/keyswitch_f64k0.o $(CSRC)/keyswitch_f64k1.o $(CSRC)/keyswitch_f64k18.o $(CSRC)/keyswitch_f64w.o $(CSRC)/keyswitch_coef.o \
           $(CSRC)/modup_mul_f64k0.o $(CSRC)/modup_mul_f64k1.o $(CSRC)/modup_mul_f64k18.o $(CSRC)/modup_mul_f64w.o \
           $(CSRC)/modup_mul2_f64k0.o $(CSRC)/modup_mul2_f64k1.o $(CSRC)/modup_mul2_f64k18.o $(CSRC)/modup_mul2_f64w.o \
           $(CSRC)/ksfold_f64k0.o $(CSRC)/ksfold_f64k1.o $(CSRC)/ksfold_f64k18.o $(CSRC)/ksfold_f64w.o \
           $(CSRC)/ksexact_f64k0.o $(CSRC)/ksexact_f64k1.o $(CSRC)/ksexact_f64k18.o $(CSRC)/ksexact_f64w.o \
           $(CSRC)/ksbgv_f64k0.o $(CSRC)/ksbgv_f64k1.o $(CSRC)/ksbgv_f64k18.o $(CSRC)/ksbgv_f64w.o \
           $(CSRC)/galois_coef.o $(CSRC)/keypair_dot2.o $(CSRC)/ct_elem.o $(CSRC)/exact_coef.o $(CSRC)/lincomb.o $(CSRC)/plain.o \
           $(CSRC)/ntt_host.o
# the kernel translation units see the kernel headers only; the host layer also the public headers
KHDRS    = $(wildcard $(CSRC)/*.h)
HDRS     = $(KHDRS) $(wildcard $(CSRC)/host/*.inc) $(wildcard include/*.h) $(wildcard include/internal/*.h)

lib: $(LIB)

$(CSRC)/ntt_host.o: $(CSRC)/ntt_host.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(CSRC)/%.o: $(CSRC)/%.hip $(KHDRS)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle all
	if [ -d /root/reference/src ]; then $(MAKE) -C oracle ref; fi

emu:
	$(MAKE) -C tests/emu -j8

all-test: lib oracle emu

clean:
	rm -f $(OBJS) $(LIB)
	$(MAKE) -C oracle clean
	$(MAKE) -C tests/emu clean

.PHONY: lib oracle emu all-test clean

# instruction-level micro-benchmarks (run on the GPU box: build/ubench)
ubench: build/ubench
build/ubench: tools/ubench.hip $(HDRS)
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -std=c++17 -ffp-contract=off -I$(CSRC) -o $@ tools/ubench.hip
.PHONY: ubench

# data-movement skeletons of the 2^14 kernel (run on the GPU box: build/skel [GiB] [launches])
skel: build/skel
build/skel: tools/skel.hip
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -std=c++17 -ffp-contract=off -o $@ tools/skel.hip
.PHONY: skel

# tensor_kernel's body with 8- and with 16-byte accesses beside a 16-byte copy (run on the GPU box: build/tensor_width [logn] [polynomials])
tensor-width: build/tensor_width
build/tensor_width: tools/tensor_width.hip $(HDRS)
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -std=c++17 -ffp-contract=off -Iinclude -Iinclude/internal -I$(CSRC) -o $@ tools/tensor_width.hip
.PHONY: tensor-width

# ASAN + UBSAN run of the CPU-side code (oracle, host table/pass planning, kernel templates in the emulator)
sanitize:
	$(MAKE) -C tests/sanitize run
.PHONY: sanitize

# memory skeleton of the XCD-local four-step transform for N = 2^16 / 2^17 (run on the GPU box: build/skel4 [GiB] [reps] [filter])
skel4: build/skel4
build/skel4: tools/skel4.hip
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -std=c++17 -ffp-contract=off -o $@ tools/skel4.hip
.PHONY: skel4

# second skeleton of the XCD-local two-pass transform: barrier-free items, class queues (build/skel5 [GiB] [reps] [filter])
skel5: build/skel5
build/skel5: tools/skel5.hip
	mkdir -p build
	$(HIPCC) -O3 --offload-arch=$(ARCH) -std=c++17 -ffp-contract=off -o $@ tools/skel5.hip
.PHONY: skel5

# what every launcher would launch, recorded instead of launched (host only, no device): for comparing two versions of the launch
# layer -- $(PROBE_OUT)/launch_probe_<pair> > file for each, the same with PROBE_CSRC=<the other csrc> PROBE_OUT=<another directory>,
# then cmp (tools/launch_probe.hip).  The probes are rebuilt on every call: which headers a program on disk was built against is not
# something make can see.
PROBE_CSRC ?= $(CSRC)
PROBE_OUT  ?= build
PROBE_PAIRS = f64k0:ArithF64:0:1 f64k1:ArithF64:1:1 f64k18:ArithF64:18:1 f64w:ArithF64W:0:1 u64:ArithU64:0:2 \
              u64x_k0:ArithU64X<0>:0:2 u64x_k1:ArithU64X<1>:1:2 u64x_k3:ArithU64X<3>:3:2 u64r4:ArithU64R4:0:3
launch-probe: $(foreach p,$(PROBE_PAIRS),$(PROBE_OUT)/launch_probe_$(firstword $(subst :, ,$(p))))
$(PROBE_OUT)/launch_probe_%: tools/launch_probe.hip FORCE
	mkdir -p $(PROBE_OUT)
	$(HIPCC) --cuda-host-only -O0 -std=c++17 -ffp-contract=off -Iinclude -Iinclude/internal -I$(PROBE_CSRC) \
	  $(foreach p,$(filter $*:%,$(PROBE_PAIRS)),'-DPROBE_POLICY=$(word 2,$(subst :, ,$(p)))' -DPROBE_KSH=$(word 3,$(subst :, ,$(p))) -DPROBE_KIND=$(word 4,$(subst :, ,$(p)))) \
	  -o $@ tools/launch_probe.hip
FORCE:
.PHONY: launch-probe FORCE
