// rt_packet_bounce.inc -- the end of a bounce of render_packet (rt_packet.inc): the Russian roulette and the next direction
// (raytracingCs.glsl :544-576), from the parked state of the bounce's hit.  Plain text, included inside a block that has `depth`
// (the bounce) and `ii` (the hit object, 0 for a lane that is not alive) in scope besides render_packet's own names: at the
// end of every iteration of the bounce loop, and in the prologue of a replaying frame's tile that resumes behind depth 0
// (DESIGN.md section 34).  One text, so that both run the very same expressions.
        const float4 mb = pk_lane_mat(sc, ii, 1);             // (roughness, diffuseStrength, ior, transparency)
        const float diffuseStrength = mb.y, ior = mb.z, transparency = mb.w;
        asm volatile("" ::: "memory");
        float *pk_ = sc.park + threadIdx.x;
        v3 thr = V3(pk_[3 * BT], pk_[4 * BT], pk_[5 * BT]);
        const v3 rd = V3(pk_[6 * BT], pk_[7 * BT], pk_[8 * BT]);
        const v3 Pb = V3(pk_[9 * BT], pk_[10 * BT], pk_[11 * BT]), Nb = V3(pk_[12 * BT], pk_[13 * BT], pk_[14 * BT]);
        const v3 Vb = V3(pk_[15 * BT], pk_[16 * BT], pk_[17 * BT]), alb = V3(pk_[18 * BT], pk_[19 * BT], pk_[20 * BT]);
        const float rough = pk_[22 * BT];
        if (depth > 2) {   // Russian roulette (:544-549)
            float dw = length(alb) * diffuseStrength;
            float cp = fminf(fmaxf(thr.x, fmaxf(thr.y, thr.z)) * 0.95f + dw, 0.99f);
            bool stop = false;
            if (alive) {
                int rx_, ry_; size_t ro_;
                pixel(rx_, ry_, ro_);
                float rnd = random2((float)((unsigned)rx_ + (unsigned)depth), (float)((unsigned)ry_ + (unsigned)depth));
                stop = rnd > cp;
            }
            if (alive && !stop) thr = div3(thr, cp);
            alive = alive && !stop;
        }
        // (alive lanes only: a dead lane gathered object 0's material)
        if constexpr (FIRST == 1) { if (alive && diffuseStrength > 0.0f) *taintWord = *taintWord | 0x100u; }
        // ---- next direction (:552-576).  Lanes whose path has ended get the same assignments (nothing reads their ray again):
        // an unconditional write keeps the old origin / direction from staying live across the whole lighting section
        Ray cur; cur.o = Pb; cur.d = rd;
        v3 nd, no;
        const float F = fresnel_schlick(fmaxf(dot(Vb, Nb), 0.0f), ior);
        if (diffuseStrength > 0.0f) {
            const int dd = depth < RT_MAX_DEPTH ? depth : RT_MAX_DEPTH - 1;
            v3 sd = reflect(rd, Nb);
            v3 hd = hemisphere_dir(V3(f.hemi[dd][0], f.hemi[dd][1], f.hemi[dd][2]), Nb);
            nd = normalize(mix_fast(sd, hd, rough));
            no = Pb + Nb * 0.001f;
            thr = thr * (alb * diffuseStrength);
        } else if (transparency > 0.0f) {
            nd = calc_refraction(cur, Nb, ior);
            no = Pb - Nb * 0.001f;
            thr = thr * ((alb * (1.0f - F)) * transparency);
        } else {
            nd = reflect(rd, Nb);
            no = Pb + Nb * 0.001f;
            thr = thr * (alb * F);
        }
        ray.d = nd; ray.o = no;
        if (alive) { pk_[3 * BT] = thr.x; pk_[4 * BT] = thr.y; pk_[5 * BT] = thr.z; }
