// Hittable.h — mirror of Source/Hittable.h:17-38.
//
// On the host the scene-graph classes are DESCRIPTORS: they carry the same public data and
// constructors as the reference's, and Camera::Render flattens them into a PrtSceneDesc for the HIP
// library (include/prt.h).  Intersection itself never runs on the host: the base Hittable::Hit /
// Occluded / Hits / ClosestPoint / Sample below forward queries to the device through the same C ABI (K1 / K7 / K6 /
// k_sample_lights).
#pragma once
#include <memory>
#include <vector>

#include "AABB.h"
#include "Math.h"

namespace Pooraytracer {

class Ray;
class Material;
class SceneFlattener;

class HitRecord {
public:
    vec3 position;
    double time = 0;
    vec3 normal; // on the same side as the ray
    vec3 tangent;
    vec2 uv;
    std::shared_ptr<Material> material;
    bool bFrontFace = false;
    void SetFaceNormal(const Ray& ray, const vec3& outwordNormal);
};

class Hittable {
public:
    virtual ~Hittable();
    // world.Hit(ray, domain, record): one-ray batch through prt_trace_closest (device).
    virtual bool Hit(const Ray& ray, Interval domain, HitRecord& record) const;
    // The batch form: every ray over the one domain in ONE launch (prt_trace_surface, device).  records is resized to
    // rays.size(); records[i] is filled from the device's record — position, time, normal, tangent, uv, bFrontFace, and the
    // hit triangle's material — where the returned [i] is true, and left default-constructed where it is not.  Not virtual.
    std::vector<bool> Hit(const std::vector<Ray>& rays, Interval domain, std::vector<HitRecord>& records) const;
    // Hit's return value where the record is not wanted (shadow, visibility, line of sight): the any-hit query,
    // prt_trace_occluded (device).  The batch form answers every ray over the one domain in ONE launch: out[i] for rays[i].
    // Not virtual: nothing overrides them, and the vtable layout of existing clients stays as it was.
    bool Occluded(const Ray& ray, Interval domain) const;
    std::vector<bool> Occluded(const std::vector<Ray>& rays, Interval domain) const;
    // The first maxHits (1..8) surfaces along the ray within the domain, nearest first, ties in the order the triangles were
    // added - the multi-hit query, prt_trace_multi (device): thickness, crossing parity, entry / exit pairs.  Fewer records
    // than maxHits: the ray has no more hits.  Each record is filled as Hit fills its one.  The batch form answers every ray
    // over the one domain in ONE launch: out[i] for rays[i].  Not virtual, as Occluded.
    std::vector<HitRecord> Hits(const Ray& ray, Interval domain, int maxHits) const;
    std::vector<std::vector<HitRecord>> Hits(const std::vector<Ray>& rays, Interval domain, int maxHits) const;
    // The point form of Hit: the point of this object's triangles nearest to p and its distance, if any lies within maxDist
    // (infinity: unbounded) - prt_closest_point (device); false, and closest / distance untouched, where none does.  The
    // batch form answers every point with the one radius in ONE launch: closest and distance are resized to p.size() and
    // filled where the returned [i] is true.  The scene keeps its triangles' corners on the device from the first use on
    // (prt_scene_set_distance_queries).  Not virtual, as Occluded.
    bool ClosestPoint(const point3& p, double maxDist, point3& closest, double& distance) const;
    std::vector<bool> ClosestPoint(const std::vector<point3>& p, double maxDist, std::vector<point3>& closest,
                                   std::vector<double>& distance) const;
    // ClosestPoint's batch form with a signed distance - prt_signed_distance (device): signedDistance[i] is negative where
    // p[i] lies inside this object, which is meaningful for a closed object whose faces are counter-clockwise seen from
    // outside (the sign is that of the angle-weighted pseudonormal of the nearest face, edge or vertex).  The scene keeps the
    // welded topology and the pseudonormals on the device from the first use on (prt_scene_set_signed_queries).  Not virtual.
    std::vector<bool> SignedDistance(const std::vector<point3>& p, double maxDist, std::vector<point3>& closest,
                                     std::vector<double>& signedDistance) const;
    // The generalized winding number of every p[i] with respect to this object - prt_winding_number (device): about 1 inside,
    // about 0 outside, and still usable (threshold 0.5) where the object is open, has seams or duplicated faces, which
    // SignedDistance's sign is not.  beta > 1 trades error for work (PRT_WINDING_BETA_DEFAULT; infinity: the exact sum).  The
    // scene keeps the moments table on the device from the first use on (prt_scene_set_winding_queries).  Not virtual.
    std::vector<double> WindingNumber(const std::vector<point3>& p, double beta = 2.0) const;
    virtual AABB BoundingBox() const = 0;
    // lights.Sample(origin, record, pdf): one sample through prt_sample_lights (device).
    virtual void Sample(const point3& origin, HitRecord& samplePointRecord, double& pdf) const;
    virtual double GetArea() const { return 0.0; }
    // Appends this object's meshes/triangles, in construction order, to the flat description.
    virtual void Flatten(SceneFlattener& out) const = 0;

private:
    struct DeviceCache;
    mutable std::shared_ptr<DeviceCache> cache_;
    friend class Camera;
    DeviceCache& Device() const;
};

} // namespace Pooraytracer
